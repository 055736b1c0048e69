"""Option "device_bvh_refit": between two full device builds, commits keep the tree's topology and refit it (csrc/hjr_bvh_build.hip,
DESIGN.md §5.1): the triangles are flattened in the current leaf order, the node boxes recomputed bottom-up over the BVH4 itself.

Frames do not depend on the tree, so every refitted frame must be the host-built context's bits.  The frame data is checked through
hjr_copy_frame_data: topology (refs rows, prim-id column) unchanged since the last full build, shading records and lights the host's
bytes, the BVH4 valid, and every used slot box the exact min / max of the triangles below it, padded: tight, not merely conservative.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from scene_util import Cornell, StressScene, hjr, new_device, ROOT
from test_device_bvh import frame_data, validate_bvh4, host_device_pair, sub_scene
from test_gpu_parity import assert_bitexact

LEAF_FLAG = 0x80000000
COUNTERS = ("samples", "closest_rays", "shadow_rays", "shaded_hits", "light_samples", "nan_samples")


def _option_json(tmp_path, extra):
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Henjou_HIP"] = extra
    p = tmp_path / "ro.json"
    p.write_text(json.dumps(ro))
    return str(p)


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_render_option_parses_device_bvh_refit(tmp_path):
    """"device_bvh_refit": N is stored as hjr_render_option.device_bvh = 1 + N (the struct does not grow); the three error cases name the key."""
    load = lambda extra: hjr.load_render_option(_option_json(tmp_path, extra))  # noqa: E731
    assert load({"device_bvh": True}).device_bvh == 1
    assert load({"device_bvh": True, "device_bvh_refit": 0}).device_bvh == 1
    assert load({"device_bvh": True, "device_bvh_refit": 8}).device_bvh == 9
    assert load({"device_bvh": 1, "device_bvh_refit": 1000}).device_bvh == 1001
    assert load({"seed": 3}).device_bvh == 0
    for bad in ({"device_bvh_refit": 8}, {"device_bvh": False, "device_bvh_refit": 8},  # without device_bvh
                {"device_bvh": True, "device_bvh_refit": 2.5}, {"device_bvh": True, "device_bvh_refit": True},  # not an integer
                {"device_bvh": True, "device_bvh_refit": 1001}, {"device_bvh": True, "device_bvh_refit": -1}):  # out of range
        with pytest.raises(hjr.HjrError, match="device_bvh_refit"):
            load(bad)


def test_stats_mirror_appends_refit_fields():
    """hjr_stats grew by bvh_refits and bvh_sah; StatsV3 mirrors them after the unchanged StatsV2 prefix."""
    assert C.sizeof(hjr.StatsV3) == C.sizeof(hjr.StatsV2) + 8
    assert hjr.StatsV3.bvh_refits.offset == C.sizeof(hjr.StatsV2) and hjr.StatsV3.bvh_sah.offset == C.sizeof(hjr.StatsV2) + 4
    assert hjr.StatsV3.bvh_builder.offset == hjr.StatsV2.bvh_builder.offset
    assert hjr.StatsV3().struct_size == C.sizeof(hjr.StatsV3)
    d = hjr.StatsV3().as_dict()
    assert {"bvh_refits", "bvh_sah", "bvh_builder", "frame_build_ms", "samples"} <= set(d) and isinstance(d["bvh_sah"], float)


# ---------------------------------------------------------------------------------------------------------------------------- GPU

def motion(arrays, k, spread=1.0):
    """Transforms of step k: instance i is rotated about y by k * (0.1 + 0.05 i) and shifted by its own translation, in front of its
    scene transform.  The inverse is computed in float64 and cast; every context gets the same arrays, so frames are comparable whatever
    the inverse's rounding."""
    m0 = np.asarray(arrays["transforms"], dtype=np.float64).reshape(-1, 3, 4)
    n = m0.shape[0]
    m, inv = np.zeros((n, 12), np.float32), np.zeros((n, 12), np.float32)
    for i in range(n):
        a = k * (0.1 + 0.05 * i)
        mv = np.eye(4)
        mv[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        mv[:3, 3] = spread * k * np.array([0.04 * ((i % 3) - 1), 0.03 * ((i % 4) - 1.5), 0.05 * ((i % 2) - 0.5)])
        full = mv @ np.vstack([m0[i], [0, 0, 0, 1]])
        m[i] = full[:3].reshape(-1).astype(np.float32)
        inv[i] = np.linalg.inv(full)[:3].reshape(-1).astype(np.float32)
    return m, inv


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def stress(tmp_path_factory):
    s = StressScene(tmp_path_factory.mktemp("refit"), spheres=8, segments=32)
    assert s.scene.view.n_triangles > 4 * 256 * 4  # several workgroups of nodes
    return s


@pytest.fixture(scope="module")
def scenes(cornell, stress):
    return {"cornell": cornell, "stress": stress}


def split_nodes(fd):
    nodes = fd["nodes"].reshape(-1, 7, 4)
    refs = nodes[:, 6, :].view(np.uint32)
    lo = np.stack([nodes[:, 0], nodes[:, 2], nodes[:, 4]], -1)  # [node, slot, axis]
    hi = np.stack([nodes[:, 1], nodes[:, 3], nodes[:, 5]], -1)
    return refs, lo, hi


def tight_boxes(fd):
    """float32 restatement of the node boxes from the copied tri_geom and refs: per used slot min / max over the triangles below it,
    -+ float32(max |coordinate|) / 8192.  min / max are exact and rounding is monotone, so padding the leaf slots and taking the
    children's min / max above them gives the bits of padding each triangle first."""
    refs, _, _ = split_nodes(fd)
    v = fd["tri_geom"].reshape(-1, 12)[:, :9].reshape(-1, 3, 3)
    pad = np.float32(np.abs(v).max()) / np.float32(8192)
    tlo, thi = v.min(1), v.max(1)
    n_nodes = refs.shape[0]
    lo = np.full((n_nodes, 4, 3), np.float32(1e30), np.float32)
    hi = np.full((n_nodes, 4, 3), np.float32(-1e30), np.float32)
    leaf = (refs & LEAF_FLAG) != 0
    used_leaf = leaf & (refs != LEAF_FLAG)
    first, count = (refs & 0x7FFFFFF).astype(np.int64), (refs >> 27) & 15
    llo = np.full((n_nodes, 4, 3), np.float32(np.inf), np.float32)
    lhi = np.full((n_nodes, 4, 3), np.float32(-np.inf), np.float32)
    for k in range(int(count[used_leaf].max())):
        sel = used_leaf & (count > k)
        llo[sel] = np.minimum(llo[sel], tlo[first[sel] + k])
        lhi[sel] = np.maximum(lhi[sel], thi[first[sel] + k])
    lo[used_leaf] = llo[used_leaf] - pad
    hi[used_leaf] = lhi[used_leaf] + pad
    for i in range(n_nodes - 1, -1, -1):  # a child's id is above its parent's
        for s in np.nonzero(~leaf[i])[0]:
            c = int(refs[i, s])
            u = refs[c] != LEAF_FLAG
            lo[i, s], hi[i, s] = lo[c][u].min(0), hi[c][u].max(0)
    return lo, hi


def sah64(fd):
    """tools/device_bvh_bench.py::bvh4_sah on copied nodes, in float64."""
    refs, lo, hi = split_nodes(fd)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    used = refs != LEAF_FLAG
    e = np.maximum(hi - lo, 0.0)
    area = 2.0 * (e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0])
    w = np.where((refs & LEAF_FLAG) != 0, 1.0 * ((refs >> 27) & 15), 1.2)
    r = np.maximum(hi[0][used[0]].max(0) - lo[0][used[0]].min(0), 0.0)
    return float((w * area)[used].sum() / (2.0 * (r[0] * r[1] + r[1] * r[2] + r[2] * r[0])))


def sah_bound(n_nodes):
    """Worst-case relative rounding error of the device's fp32 cost against exact arithmetic on the same nodes, u = 2^-24.  All terms
    are non-negative, so the factors (1 + d), |d| <= u, of every operation on the way of a term bound the whole sum:
      slot area 6 (three extents, a product of two of them, two additions; the doubling is exact), weight 2 (Ci = 1.2f is not 1.2; the
      product), the node's sum over its slots 4, the lane's sum over its ceil(ceil(n / 256) / 256) nodes, the workgroup's tree 8 (six
      shuffle levels, two levels over the four waves), the same tree over the 256 partial sums 8, the root's area 6, the division 1."""
    u = 2.0 ** -24
    chunk = (n_nodes + 255) // 256   # nodes per workgroup
    lane = (chunk + 255) // 256      # of them per lane
    ops = 6 + 2 + 4 + lane + 8 + 8 + 6 + 1
    return 1.01 * ops * u  # 1.01: the second-order terms of (1 + u)^ops


def bits(x):
    return np.float32(x).view(np.uint32)


def check_refitted_frame_data(scene, dev, host, base, leaf_max=2):
    """The frame data of a refitted (or rebuilt) device context against the host's and against the last full build `base`."""
    n = scene.scene.view.n_triangles
    fd, fh = frame_data(dev), frame_data(host)
    if base is not None:
        assert split_nodes(fd)[0].tobytes() == split_nodes(base)[0].tobytes(), "refs rows changed"
        assert fd["tri_geom"].reshape(-1, 12)[:, 9].tobytes() == base["tri_geom"].reshape(-1, 12)[:, 9].tobytes(), "leaf order changed"
    assert fd["tri_shade"].tobytes() == fh["tri_shade"].tobytes()
    assert fd["lights"].tobytes() == fh["lights"].tobytes()
    gd, gh = fd["tri_geom"].reshape(-1, 12), fh["tri_geom"].reshape(-1, 12)
    idd, idh = gd[:, 9].view(np.uint32), gh[:, 9].view(np.uint32)
    assert np.array_equal(np.sort(idd), np.arange(n, dtype=np.uint32))
    assert gd[np.argsort(idd)].tobytes() == gh[np.argsort(idh)].tobytes(), "tri_geom is not a row permutation of the host's"
    validate_bvh4(fd, n, leaf_max, dev.stats()["stack_need"])
    refs, lo, hi = split_nodes(fd)
    elo, ehi = tight_boxes(fd)
    used = refs != LEAF_FLAG
    assert lo[used].tobytes() == elo[used].tobytes() and hi[used].tobytes() == ehi[used].tobytes(), "slot boxes are not the tight padded boxes"
    return fd


def check_frames(scene, dev, host, what, integrator=hjr.INTEGRATOR_NEE, w=64, h=48, spp=4):
    """Colour, albedo and normal of both contexts bit for bit; under NEE with HJR_FLAG_STATS, and the tree-independent counters equal."""
    counted = integrator == hjr.INTEGRATOR_NEE
    p = scene.hjr_params(w, h, spp, flags=hjr.FLAG_STATS if counted else 0, integrator=integrator)
    a = dev.render(p)
    sd = dev.stats()
    b = host.render(p)
    sh = host.stats()
    for x, y, aov in zip(a, b, ("colour", "albedo", "normal")):
        assert_bitexact(x, y, "%s (%s)" % (what, aov))
    for k in COUNTERS if counted else ():
        assert sd[k] == sh[k], (what, k, sd[k], sh[k])
    return b


@pytest.mark.gpu
def test_options_round_trip_and_host_builder_ignores_them(cornell):
    d = new_device()
    try:
        for key, hi in (("device_bvh_refit", 1000), ("device_bvh_refit_growth", 10000)):
            assert d.get_option(key) == -1
            for v in (0, 7, hi):
                d.set_option(key, v)
                assert d.get_option(key) == v
            for bad in (hi + 1, -2):
                with pytest.raises(hjr.HjrError):
                    d.set_option(key, bad)
    finally:
        d.close()
    a = cornell.device({"lds_bvh": 0, "bvh_width": 4, "device_bvh": 0, "device_bvh_refit": 4, "force_rebuild": 1})
    b = cornell.device({"lds_bvh": 0, "bvh_width": 4})
    try:
        a.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
        st = a.stats()
        assert st["bvh_builder"] == 0 and st["bvh_refits"] == 0 and st["bvh_sah"] == 0.0
        fa, fb = frame_data(a), frame_data(b)
        for k in fa:
            assert fa[k].tobytes() == fb[k].tobytes(), k
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("leaf_max", [1, 2, 4])
@pytest.mark.parametrize("opt", [0, 1])
@pytest.mark.parametrize("name", ["cornell", "stress"])
def test_refit_with_unchanged_transforms_is_the_full_build(scenes, name, opt, leaf_max):
    s = scenes[name]
    d = s.device({"device_bvh": 1, "device_bvh_opt": opt, "leaf_max": leaf_max})
    try:
        full, sf = frame_data(d), d.stats()
        assert sf["bvh_builder"] == 1 and sf["bvh_refits"] == 0 and sf["bvh_sah"] > 0
        d.set_option("force_rebuild", 1)
        d.set_option("device_bvh_refit", 4)
        d.set_transforms(s.arrays["transforms"], s.arrays["inv_transforms"])
        fd, sr = frame_data(d), d.stats()
        assert sr["bvh_refits"] == 1 and sr["bvh_builder"] == 1 and sr["frame_build_ms"] > 0
        for k in ("nodes", "tri_geom", "tri_shade", "lights"):
            assert fd[k].tobytes() == full[k].tobytes(), "%s differs from the full build's" % k
        for k in ("bvh_nodes", "bvh_depth", "stack_need"):
            assert sr[k] == sf[k], k
        assert bits(sr["bvh_sah"]) == bits(sf["bvh_sah"])
    finally:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "stress"])
def test_animated_sequence(scenes, name):
    s = scenes[name]
    dev, host = host_device_pair(s, device_bvh_opt=1)
    try:
        dev.set_option("device_bvh_refit", 4)
        dev.set_option("device_bvh_refit_growth", 10000)
        base = frame_data(dev)
        for k in range(1, 6):
            m, inv = motion(s.arrays, k)
            dev.set_transforms(m, inv)
            host.set_transforms(m, inv)
            st = dev.stats()
            assert st["bvh_refits"] == (k if k <= 4 else 0), (k, st["bvh_refits"])
            assert st["bvh_builder"] == 1
            check_frames(s, dev, host, "%s, commit %d" % (name, k))
            if k == 2:
                check_frames(s, dev, host, "%s, commit %d, MIS" % (name, k), integrator=hjr.INTEGRATOR_MIS)
            fd = check_refitted_frame_data(s, dev, host, base if k <= 4 else None)
            p = s.hjr_params(64, 48, 1)
            assert dev.gbuffer(p).tobytes() == host.gbuffer(p).tobytes(), "G-buffer (tri_inst) differs at commit %d" % k
            if k == 5:
                base = fd
    finally:
        dev.close()
        host.close()


def guard_motion(arrays, amount, turn=0.0):
    """The guard run's motion: the instance with the largest world box stays; the others change places (instance j moves `amount` of the
    way to the centre of the next one, cyclically) while turning about y through their own centres, so that they pass through each
    other inside a root box that hardly changes (the cost is relative to the root's area)."""
    m0 = np.asarray(arrays["transforms"], dtype=np.float64).reshape(-1, 3, 4)
    v = np.asarray(arrays["vertices"], dtype=np.float64).reshape(-1, 3)
    idx = np.asarray(arrays["indices"], dtype=np.int64).reshape(-1, 3)
    po = list(np.asarray(arrays["prim_offsets"], dtype=np.int64)) + [idx.shape[0]]
    n = m0.shape[0]
    centre, size = np.zeros((n, 3)), np.zeros(n)
    for i in range(n):
        w = v[idx[po[i]:po[i + 1]].reshape(-1)] @ m0[i][:, :3].T + m0[i][:, 3]
        centre[i], size[i] = 0.5 * (w.min(0) + w.max(0)), np.linalg.norm(w.max(0) - w.min(0))
    movers = [i for i in range(n) if i != int(np.argmax(size))]
    m, inv = np.zeros((n, 12), np.float32), np.zeros((n, 12), np.float32)
    for i in range(n):
        mv = np.eye(4)
        if i in movers:
            j = movers[(movers.index(i) + 1) % len(movers)]
            a = turn + amount * (0.5 + 0.3 * i)
            mv[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
            mv[:3, 3] = centre[i] + amount * (centre[j] - centre[i]) - mv[:3, :3] @ centre[i]
        full = mv @ np.vstack([m0[i], [0, 0, 0, 1]])
        m[i] = full[:3].reshape(-1).astype(np.float32)
        inv[i] = np.linalg.inv(full)[:3].reshape(-1).astype(np.float32)
    return m, inv


# Enlarged until both scenes grow by at least 5 %.  Measured on an MI355X (device_bvh_opt 1), growth of the refitted tree's cost at
# amount 0.25 / 0.5 / 0.75: Cornell box +3.4 / +6.3 / +10.6 % (9.572 -> 10.586), stress scene +0.8 / +2.5 / +7.4 % (8.750 -> 9.395).
# At 1.0 every mover sits in another one's place and the tree is tight again (+1.1 / +5.0 %).
GUARD_AMOUNT = 0.75


def check_cost(name, dev):
    st = dev.stats()
    ref = sah64(frame_data(dev))
    bound = sah_bound(st["bvh_nodes"])
    print("%s: bvh_sah %.9g, float64 %.9g, relative error %.3g, bound %.3g" % (name, st["bvh_sah"], ref, abs(st["bvh_sah"] - ref) / ref, bound))
    assert bound <= 1e-3
    assert abs(st["bvh_sah"] - ref) <= bound * ref
    return st["bvh_sah"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "stress"])
def test_tree_cost_and_growth_guard(scenes, name):
    s = scenes[name]
    options = {"device_bvh": 1, "device_bvh_opt": 1, "device_bvh_refit": 4}
    devs = [s.device(dict(options, device_bvh_refit_growth=10000)), s.device({"lds_bvh": 0, "bvh_width": 4})]
    dev, host = devs
    try:
        m, inv = guard_motion(s.arrays, GUARD_AMOUNT)
        host.set_transforms(m, inv)
        s0 = check_cost(name + ", build", dev)
        dev.set_transforms(m, inv)
        s1 = check_cost(name + ", refit", dev)
        print("%s: s0 %.6g, s1 %.6g, growth %.1f %%" % (name, s0, s1, 100.0 * (s1 / s0 - 1.0)))
        assert dev.stats()["bvh_refits"] == 1
        # the motion pulls the instances through each other: the refitted tree must cost at least 5 % more than the build
        assert s1 >= 1.05 * s0, (s0, s1)
        check_frames(s, dev, host, "%s, refit past the guard's growth" % name)
        growth = int(100.0 * (s1 / s0 - 1.0) / 2.0)
        dev = s.device(dict(options, device_bvh_refit_growth=growth))
        devs.append(dev)
        dev.set_transforms(m, inv)
        assert dev.stats()["bvh_refits"] == 1  # the tripping refit is valid and stays current
        check_frames(s, dev, host, "%s, tripping refit" % name)
        m2, inv2 = guard_motion(s.arrays, GUARD_AMOUNT, turn=0.2)
        dev.set_transforms(m2, inv2)
        host.set_transforms(m2, inv2)
        assert dev.stats()["bvh_refits"] == 0, "the commit after a refit that tripped the guard must be a full build"
        check_frames(s, dev, host, "%s, rebuild after the guard" % name)
        dev.set_option("force_rebuild", 1)
        dev.set_transforms(m2, inv2)
        assert dev.stats()["bvh_refits"] == 1  # refits resume after it
    finally:
        for d in devs:
            d.close()


@pytest.mark.gpu
def test_failed_refit_keeps_the_previous_frame(cornell):
    dev, host = host_device_pair(cornell)
    try:
        dev.set_option("device_bvh_refit", 8)
        m, inv = motion(cornell.arrays, 1)
        dev.set_transforms(m, inv)
        host.set_transforms(m, inv)
        assert dev.stats()["bvh_refits"] == 1
        good = check_frames(cornell, dev, host, "refit before the failure")
        bad = m.copy()
        bad[0, 0] = np.nan
        with pytest.raises(hjr.HjrError, match="non-finite vertex after transform") as e:
            dev.set_transforms(bad, inv)  # would have been refit 2
        assert "(-1)" in str(e.value)  # HJR_ERR_ARG
        p = cornell.hjr_params(64, 48, 4, flags=hjr.FLAG_STATS)
        for x, y in zip(dev.render(p), good):
            assert_bitexact(x, y, "previous frame after a failed refit")
        m, inv = motion(cornell.arrays, 2)
        dev.set_transforms(m, inv)
        host.set_transforms(m, inv)
        assert dev.stats()["bvh_refits"] == 2
        check_frames(cornell, dev, host, "refit after the failure")
        check_refitted_frame_data(cornell, dev, host, None)
    finally:
        dev.close()
        host.close()


@pytest.mark.gpu
def test_what_makes_the_next_commit_a_full_build(cornell):
    dev, host = host_device_pair(cornell)
    step = [0]

    def commit(expect, what):
        step[0] += 1
        m, inv = motion(cornell.arrays, step[0])
        dev.set_transforms(m, inv)
        host.set_transforms(m, inv)
        assert dev.stats()["bvh_refits"] == expect, what
        check_frames(cornell, dev, host, what)

    try:
        dev.set_option("device_bvh_refit", 100)
        commit(1, "refit")
        dev.set_option("leaf_max", 4)
        host.set_option("leaf_max", 4)
        commit(0, "leaf_max changed")
        check_refitted_frame_data(cornell, dev, host, None, leaf_max=4)
        commit(1, "refit of the leaf_max 4 tree")
        check_refitted_frame_data(cornell, dev, host, None, leaf_max=4)
        dev.set_option("device_bvh_opt", 1)
        commit(0, "device_bvh_opt changed")
        commit(1, "refit of the restructured tree")
        dev.upload_scene(cornell.scene.view)
        host.upload_scene(cornell.scene.view)
        commit(0, "new hjr_upload_scene")
        commit(1, "refit after the upload's build")
        dev.set_option("device_bvh", 0)
        dev.set_option("lds_bvh", 0)
        dev.set_option("bvh_width", 4)
        step[0] += 1
        dev.set_transforms(*motion(cornell.arrays, step[0]))
        assert dev.stats()["bvh_builder"] == 0 and dev.stats()["bvh_refits"] == 0 and dev.stats()["bvh_sah"] == 0.0
        dev.set_option("device_bvh", 1)
        commit(0, "host-built data -> device_bvh 1")
        commit(1, "refit after it")
    finally:
        dev.close()
        host.close()


@pytest.mark.gpu
def test_tiny_scenes_with_refit_on(cornell):
    arrays = cornell.arrays
    lights = set(int(t) for t in arrays["light_prim_ids"])
    others = [t for t in range(cornell.scene.view.n_triangles) if t not in lights]
    p = cornell.hjr_params(48, 32, 4, integrator=hjr.INTEGRATOR_MIS)
    for k in (0, 1, 2):
        a = sub_scene(arrays, ([min(lights)] + others[:k - 1]) if k else [])
        dev, host = new_device({"device_bvh": 1, "device_bvh_refit": 4, "device_bvh_refit_growth": 10000}), new_device({"lds_bvh": 0, "bvh_width": 4})
        try:
            for d in (dev, host):
                d.upload_arrays(a)
                d.set_transforms(a["transforms"], a["inv_transforms"])
            for step in (1, 2):
                m, inv = motion(a, step)
                dev.set_transforms(m, inv)
                host.set_transforms(m, inv)
                assert dev.stats()["bvh_refits"] == (step if k >= 2 else 0), (k, step)
                for x, y, aov in zip(dev.render(p), host.render(p), ("colour", "albedo", "normal")):
                    assert_bitexact(x, y, "%d triangles, commit %d (%s)" % (k, step, aov))
        finally:
            dev.close()
            host.close()


@pytest.mark.gpu
def test_cli_refit_same_pngs(tmp_path):
    cli = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
    pngs, errs = [], []
    for refit in (False, True):
        work = tmp_path / ("run%d" % refit)
        shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
        ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
        ro["Image"].update(image_width=96, image_height=64, max_spp=8, image_name="refit")
        ro["Animation"].update(start_frame=1, end_frame=4)
        ro["Henjou_HIP"] = {"seed": 5, "device_bvh": True, "force_rebuild": True, "verbose": True}
        if refit:
            ro["Henjou_HIP"]["device_bvh_refit"] = 8
        (work / "render_option.json").write_text(json.dumps(ro))
        (work / "fps.txt").write_text("24")
        p = subprocess.run([cli, "render_option.json"], cwd=work, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        pngs.append([(work / ("refit_%03d.png" % f)).read_bytes() for f in (1, 2, 3)])
        errs.append([ln for ln in p.stderr.splitlines() if "device build" in ln or "device refit" in ln])
    assert pngs[0] == pngs[1]
    assert ["device refit" in ln for ln in errs[0]] == [False, False, False], errs[0]
    assert ["device refit" in ln for ln in errs[1]] == [False, True, True], errs[1]
