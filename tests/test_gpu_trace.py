"""Ray-level traversal tests: hjr_trace_rays hands the product's traversal rays of the test's own choosing — the adversarial classes of
tests/trace_util.py — and every result (occluded, prim, t, b1, b2) is compared BIT FOR BIT with the oracle's brute force over all
triangles, for every kernel layout and both traversal loops (stand-alone and fused; the wavefront trace stage is not reachable through the
hook, include/henjou_hip.h).  No tolerance, no excluded ray.  The inputs are pinned on the CPU by tests/test_trace_rays_host.py."""
import numpy as np
import pytest

import trace_util as tu
from scene_util import Cornell, hjr, new_device

pytestmark = pytest.mark.gpu

PATHS = {"standalone": hjr.TRACE_STANDALONE, "fused": hjr.TRACE_FUSED}
MEM2 = dict(lds_bvh=0, bvh_width=2)
# name -> (options, expected hjr_stats.lds_mode, overflow pushes expected)
SOUP_CONFIGS = {
    "default": ({}, None, False),
    "stack16": (dict(lds_stack16=1), 2, False),
    "bvh2_mem": (MEM2, 3, False),
    "bvh4_top0": (dict(bvh_width=4, top_nodes=0), 0, False),
    "bvh4": (dict(bvh_width=4), 0, False),
    "bvh2_mem_short2": (dict(MEM2, short_stack=2), 3, True),
    "bvh4_short2": (dict(bvh_width=4, short_stack=2), 0, True),
    "leaf1": (dict(leaf_max=1), None, False),
    "leaf4": (dict(leaf_max=4), None, False),
    "node_min1": (dict(node_min=1), None, False),
    "node_min64": (dict(node_min=64), None, False),
    "device_bvh": (dict(device_bvh=1), 0, False),
    "device_bvh_opt": (dict(device_bvh=1, device_bvh_opt=1), 0, False),
}
OTHER_CONFIGS = {"default": ({}, None, False), "bvh4": (dict(bvh_width=4), 0, False)}

_batches = {}


def batch_of(scene):
    """the scene's arrays and its batch with the brute-force reference, computed once"""
    if scene not in _batches:
        if scene == "soup":
            a = tu.soup_arrays()
        elif scene == "offset":
            a = tu.soup_arrays(tu.OFFSET)
        else:
            a = Cornell().arrays
        grid = None if scene == "cornell" else np.arange(tu.GRID_FIRST, tu.GRID_FIRST + tu.GRID_COUNT)
        b = tu.Batch(a, grid=grid)
        b.ref, b.ref8  # noqa: B018
        _batches[scene] = (a, b)
    return _batches[scene]


def class_of(b, idx):
    return [k for k, s in b.slices.items() if s.start <= idx < s.stop][0]


def check(dev, path, shadow, closest, ref, what, b=None, order=None, tri_prim=None):
    got = dev.trace_rays(path, shadow, closest)
    assert (got["status"] == hjr.TRACE_STATUS_OK).all(), (what, np.unique(got["status"], return_counts=True))
    bad = tu.mismatches(got, ref)
    if bad.size:
        rows = []
        for i in bad[:8]:
            src = int(order[i]) if order is not None else int(i)
            rows.append((class_of(b, src) if b is not None and src < b.n else "?", src, got[i], ref[i], shadow[i], closest[i]))
        pytest.fail("%s: %d of %d pairs differ from the brute force; first: %s" % (what, bad.size, got.size, rows))
    if tri_prim is not None:  # the row at tri_geom[k] carries prim
        hit = got["prim"] != tu.NO_PRIM
        assert np.array_equal(tri_prim[got["k"][hit]], got["prim"][hit]), what
        assert (got["k"][~hit] == 0).all()
    return got


def run_config(scene, options, expect_mode, expect_overflow, path_name):
    """one device under `options`: every submission order and size of the scene's batch on one traversal loop"""
    arrays, b = batch_of(scene)
    path = PATHS[path_name]
    dev = new_device(options)
    try:
        dev.upload_arrays(arrays)
        dev.set_transforms(arrays["transforms"], arrays["inv_transforms"])
        tri_prim = dev.copy_frame_data(hjr.FRAME_TRI_GEOM).view(np.uint32).reshape(-1, 12)[:, 9]
        assert dev.trace_rays(path, b.shadow[:0], b.closest[:0]).size == 0  # n == 0 does nothing
        # in class order
        exact = check(dev, path, b.shadow, b.closest, b.ref, "class order", b, None, tri_prim)
        st = dev.stats()
        print("%s %s %s: lds_mode %d, stack %d / %d" % (scene, options, path_name, st["lds_mode"], st["stack_lds_entries"], st["stack_need"]))
        if expect_mode is not None:
            assert st["lds_mode"] == expect_mode, st
        if expect_overflow:
            assert st["stack_need"] > st["stack_lds_entries"] == 2, st
            assert st["stack_overflow_pushes"] > 0, "the overflow branch of LaneStack::put never ran"
            print("%s %s %s: %d overflow pushes" % (scene, options, path_name, st["stack_overflow_pushes"]))
        # the approximate-arithmetic build of the same kernels: the same bits, record for record
        fast = dev.trace_rays(path | hjr.TRACE_FAST_BUILD, b.shadow, b.closest)
        assert np.array_equal(fast.view(np.uint32), exact.view(np.uint32)), "HJR_TRACE_FAST_BUILD differs from the exact build in %d records" % int(
            (fast.view(np.uint32).reshape(-1, 8) != exact.view(np.uint32).reshape(-1, 8)).any(1).sum())
        # shuffled across classes: the lanes of a wave hold unlike rays
        order = np.random.default_rng(11).permutation(b.n)
        sh, cl, ref = b.shadow[order], b.closest[order], b.ref[order]
        shuffled = check(dev, path, sh, cl, ref, "shuffled", b, order, tri_prim)
        fast = dev.trace_rays(path | hjr.TRACE_FAST_BUILD, sh, cl)
        assert np.array_equal(fast.view(np.uint32), shuffled.view(np.uint32)), "HJR_TRACE_FAST_BUILD differs from the exact build on the shuffled batch"
        # valid flags mixed: both rays, shadow only, closest only, neither
        sv, cv = tu.valid_mix(b.n)
        shm, clm = sh.copy(), cl.copy()
        shm["valid"], clm["valid"] = sv, cv
        check(dev, path, shm, clm, tu.masked_ref(ref, sv, cv), "valid flags mixed", b, order, tri_prim)
        for n in (1, 63, 64, 65):
            check(dev, path, shm[:n], clm[:n], tu.masked_ref(ref, sv, cv)[:n], "n = %d" % n, b, order, tri_prim)
            check(dev, path, sh[100:100 + n], cl[100:100 + n], ref[100:100 + n], "n = %d, all valid" % n, b, order[100:], tri_prim)
        # one wave's worth of non-finite rays, last and in a call of its own: no hit, not occluded, every pair resolved
        got8 = check(dev, path, b.shadow8, b.closest8, b.ref8, "non-finite rays")
        assert (got8["prim"] == tu.NO_PRIM).all() and (got8["occluded"] == 0).all()
    finally:
        dev.close()


@pytest.mark.parametrize("path_name", list(PATHS))
@pytest.mark.parametrize("config", list(SOUP_CONFIGS))
def test_hostile_soup(config, path_name):
    options, mode, overflow = SOUP_CONFIGS[config]
    run_config("soup", options, mode, overflow, path_name)


@pytest.mark.parametrize("path_name", list(PATHS))
@pytest.mark.parametrize("config", list(OTHER_CONFIGS))
@pytest.mark.parametrize("scene", ["cornell", "offset"])
def test_cornell_and_offset_soup(scene, config, path_name):
    """the bundled scene, and the soup at (1000, -500, 250): large max |coord|, box padding and slab-test precision at scale, far origins at
    64 x that (the supported bound of DESIGN.md 4.3)"""
    options, mode, overflow = OTHER_CONFIGS[config]
    run_config(scene, options, mode, overflow, path_name)


def test_argument_errors_come_before_any_launch():
    arrays, b = batch_of("soup")
    dev = new_device()
    try:
        L = hjr.lib()
        out = np.zeros(4, hjr.RAY_RESULT_DTYPE)
        sh, cl = np.ascontiguousarray(b.shadow[:4]), np.ascontiguousarray(b.closest[:4])
        # no frame data yet
        assert L.hjr_trace_rays(dev._h, hjr.TRACE_FUSED, 4, sh.ctypes.data, cl.ctypes.data, out.ctypes.data) == -5
        assert L.hjr_trace_rays(dev._h, hjr.TRACE_FUSED, 0, None, None, None) == -5
        dev.upload_arrays(arrays)
        dev.set_transforms(arrays["transforms"], arrays["inv_transforms"])
        assert L.hjr_trace_rays(dev._h, hjr.TRACE_WAVEFRONT, 4, sh.ctypes.data, cl.ctypes.data, out.ctypes.data) == -1
        assert L.hjr_trace_rays(dev._h, 5, 4, sh.ctypes.data, cl.ctypes.data, out.ctypes.data) == -1
        assert L.hjr_trace_rays(dev._h, hjr.TRACE_STANDALONE, 4, sh.ctypes.data, None, out.ctypes.data) == -1
        assert (out.view(np.uint32) == 0).all()
        assert L.hjr_trace_rays(dev._h, hjr.TRACE_STANDALONE, 0, None, None, None) == 0
    finally:
        dev.close()
