"""Option "device_bvh_instances": per-instance trees built once per uploaded scene, a top tree over the instances' world boxes at every
commit (csrc/hjr_bvh_build.hip).  Triangles stay flattened to world space and one BVH4 is emitted, so every frame must
be the host-built context's bits.  The frame data is checked through hjr_copy_frame_data: a valid BVH4 with tight padded boxes, the
instances as contiguous tri_geom row blocks in instance order, no slot that cuts through an instance unless it lies inside one, and
bytes that depend on the current transforms only, never on the commits before.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import trace_util as tu
from scene_util import Cornell, StressScene, hjr, new_device, ROOT
from table_util import TableScene
from test_device_bvh import frame_data, validate_bvh4, host_device_pair, sub_scene, same_place_scene
from test_device_bvh_refit import motion, split_nodes, tight_boxes, sah64, sah_bound, check_frames
from test_gpu_parity import assert_bitexact

LEAF_FLAG = 0x80000000
HOST = {"lds_bvh": 0, "bvh_width": 4}
TOP_MAX = 1024  # csrc/hjr_bvh_build.h::HJR_TOP_MAX


def _option_json(tmp_path, extra):
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Henjou_HIP"] = extra
    p = tmp_path / "ro.json"
    p.write_text(json.dumps(ro))
    return str(p)


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_render_option_parses_device_bvh_instances(tmp_path):
    """"device_bvh_instances": true is bit 8 of hjr_render_option.device_bvh_opt, whose low bits stay the rounds; the four error cases
    name the key."""
    load = lambda extra: hjr.load_render_option(_option_json(tmp_path, extra))  # noqa: E731
    o = load({"device_bvh": True, "device_bvh_instances": True})
    assert o.device_bvh == 1 and o.device_bvh_opt & 0xff == 0 and o.device_bvh_opt >> 8 == 1
    o = load({"device_bvh": True, "device_bvh_opt": 2, "device_bvh_instances": True})
    assert o.device_bvh_opt & 0xff == 2 and o.device_bvh_opt >> 8 == 1
    assert load({"device_bvh": True, "device_bvh_opt": 3, "device_bvh_instances": 1}).device_bvh_opt == 0x103
    assert load({"device_bvh": True, "device_bvh_opt": 3}).device_bvh_opt == 3
    assert load({"device_bvh": True, "device_bvh_opt": 1, "device_bvh_instances": False}).device_bvh_opt == 1
    assert load({"device_bvh": True, "device_bvh_instances": 0}).device_bvh_opt == 0
    assert load({"device_bvh": True, "device_bvh_refit": 8, "device_bvh_instances": True}).device_bvh == 9
    for bad in ({"device_bvh_instances": True}, {"device_bvh": False, "device_bvh_instances": True},
                {"device_bvh": True, "device_bvh_instances": "yes"}, {"device_bvh": True, "device_bvh_instances": 2}):
        with pytest.raises(hjr.HjrError, match="device_bvh_instances"):
            load(bad)


def test_stats_mirror_appends_instance_fields():
    """hjr_stats grew by bvh_instances and bvh_topology_ms; StatsV4 mirrors them after the unchanged StatsV3 prefix."""
    assert C.sizeof(hjr.StatsV4) == C.sizeof(hjr.StatsV3) + 8
    assert hjr.StatsV4.bvh_instances.offset == C.sizeof(hjr.StatsV3) and hjr.StatsV4.bvh_topology_ms.offset == C.sizeof(hjr.StatsV3) + 4
    assert hjr.StatsV4.bvh_refits.offset == hjr.StatsV3.bvh_refits.offset and hjr.StatsV4.bvh_sah.offset == hjr.StatsV3.bvh_sah.offset
    assert hjr.StatsV4().struct_size == C.sizeof(hjr.StatsV4)
    d = hjr.StatsV4().as_dict()
    assert {"bvh_instances", "bvh_topology_ms", "bvh_refits", "bvh_sah", "samples"} <= set(d)
    assert isinstance(d["bvh_topology_ms"], float) and isinstance(d["bvh_instances"], int)


# ---------------------------------------------------------------------------------------------------------------------------- GPU

def bits(x):
    return np.float32(x).view(np.uint32)


def n_tris_of(arrays):
    return np.asarray(arrays["indices"]).size // 3


def instance_sizes(arrays):
    po = np.asarray(arrays["prim_offsets"], dtype=np.int64).reshape(-1)
    return np.diff(np.append(po, n_tris_of(arrays)))


def non_empty(arrays):
    return int((instance_sizes(arrays) > 0).sum())


def prim_instance(arrays, prims):
    """prim_offset maps a prim to its instance: the last instance whose offset is <= the prim"""
    po = np.asarray(arrays["prim_offsets"], dtype=np.int64).reshape(-1)
    return np.searchsorted(po, np.asarray(prims, dtype=np.int64), side="right") - 1


def check_data(arrays, dev, host, leaf_max=2, partition=True):
    """The frame data of an instance-built context: valid, tight, the host's records, cost within the fp32 bound; returns it."""
    n = n_tris_of(arrays)
    st = dev.stats()
    fd, fh = frame_data(dev), frame_data(host)
    validate_bvh4(fd, n, leaf_max, st["stack_need"])
    refs, lo, hi = split_nodes(fd)
    elo, ehi = tight_boxes(fd)
    used = refs != LEAF_FLAG
    assert lo[used].tobytes() == elo[used].tobytes() and hi[used].tobytes() == ehi[used].tobytes(), "slot boxes are not the tight padded boxes"
    assert fd["tri_shade"].tobytes() == fh["tri_shade"].tobytes()
    assert fd["lights"].tobytes() == fh["lights"].tobytes()
    gd, gh = fd["tri_geom"].reshape(-1, 12), fh["tri_geom"].reshape(-1, 12)
    idd, idh = gd[:, 9].view(np.uint32), gh[:, 9].view(np.uint32)
    assert np.array_equal(np.sort(idd), np.arange(n, dtype=np.uint32))
    assert gd[np.argsort(idd)].tobytes() == gh[np.argsort(idh)].tobytes(), "tri_geom is not a row permutation of the host's"
    ref, bound = sah64(fd), sah_bound(st["bvh_nodes"])
    assert abs(st["bvh_sah"] - ref) <= bound * ref, (st["bvh_sah"], ref, bound)
    if partition:
        check_partition(arrays, fd)
    return fd


def check_partition(arrays, fd):
    """Instances are contiguous row blocks in instance order; the triangles below a slot lie in one instance or are whole instances."""
    sizes = instance_sizes(arrays)
    row_inst = prim_instance(arrays, fd["tri_geom"].reshape(-1, 12)[:, 9].view(np.uint32))
    assert np.all(np.diff(row_inst) >= 0), "instance blocks are not contiguous and in instance order"
    refs, _, _ = split_nodes(fd)
    n_nodes, n_inst = refs.shape[0], sizes.size
    below = np.zeros((n_nodes, 4, n_inst), dtype=np.int64)  # triangles of each instance below each slot
    leaf = (refs & LEAF_FLAG) != 0
    for i in range(n_nodes - 1, -1, -1):  # a child's id is above its parent's
        for s in range(4):
            r = int(refs[i, s])
            if r == LEAF_FLAG:
                continue
            if leaf[i, s]:
                f, c = r & 0x7FFFFFF, (r >> 27) & 15
                below[i, s] = np.bincount(row_inst[f:f + c], minlength=n_inst)
            else:
                below[i, s] = below[r].sum(0)
    touched = below > 0
    several = touched.sum(-1) > 1
    whole = np.all(~touched | (below == sizes), axis=-1)
    assert np.all(~several | whole), "%d slots cut through an instance while holding another one" % int((several & ~whole).sum())
    assert np.array_equal(below[0].sum(0), sizes)


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def stress(tmp_path_factory):
    s = StressScene(tmp_path_factory.mktemp("inst"), spheres=8, segments=32)
    assert s.scene.view.n_triangles > 4 * 256 * 4 and non_empty(s.arrays) >= 8  # several workgroups of nodes
    return s


@pytest.fixture(scope="module")
def scenes(cornell, stress):
    return {"cornell": cornell, "stress": stress}


def instance_pair(scene, **opts):
    return host_device_pair(scene, device_bvh_instances=1, **opts)


def commit(devs, m, inv):
    for d in devs:
        d.set_transforms(m, inv)


def close(*devs):
    for d in devs:
        d.close()


@pytest.mark.gpu
def test_option_round_trip_and_harmless_without_device_bvh(cornell):
    d = new_device()
    try:
        assert d.get_option("device_bvh_instances") == -1
        for v in (0, 1):
            d.set_option("device_bvh_instances", v)
            assert d.get_option("device_bvh_instances") == v
        for bad in (2, -2):
            with pytest.raises(hjr.HjrError):
                d.set_option("device_bvh_instances", bad)
    finally:
        d.close()
    a, b = cornell.device(dict(HOST, device_bvh_instances=1, force_rebuild=1)), cornell.device(HOST)
    try:
        a.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
        st = a.stats()
        assert st["bvh_builder"] == 0 and st["bvh_instances"] == 0 and st["bvh_topology_ms"] == 0.0
        fa, fb = frame_data(a), frame_data(b)
        for k in fa:
            assert fa[k].tobytes() == fb[k].tobytes(), k
    finally:
        close(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [0, 1])
@pytest.mark.parametrize("name", ["cornell", "stress"])
def test_animated_frames_and_frame_data(scenes, name, opt):
    s = scenes[name]
    dev, host = instance_pair(s, device_bvh_opt=opt)
    try:
        prims = None
        for k in range(6):
            commit((dev, host), *motion(s.arrays, k))
            st = dev.stats()
            assert st["bvh_instances"] == non_empty(s.arrays) and st["bvh_refits"] == 0 and st["bvh_builder"] == 1, (k, st)
            check_frames(s, dev, host, "%s, opt %d, step %d" % (name, opt, k))
            if k == 2:
                check_frames(s, dev, host, "%s, step %d, MIS" % (name, k), integrator=hjr.INTEGRATOR_MIS)
            if k == 4:
                check_frames(s, dev, host, "%s, step %d, Pathtrace" % (name, k), integrator=hjr.INTEGRATOR_PT)
            fd = check_data(s.arrays, dev, host)
            col = fd["tri_geom"].reshape(-1, 12)[:, 9].tobytes()
            assert prims is None or col == prims, "the leaf order changed at step %d" % k
            prims = col
            p = s.hjr_params(64, 48, 1)
            assert dev.gbuffer(p).tobytes() == host.gbuffer(p).tobytes(), "G-buffer (tri_inst) differs at step %d" % k
    finally:
        close(dev, host)


@pytest.mark.gpu
@pytest.mark.parametrize("leaf_max", [1, 4])
def test_leaf_max(stress, leaf_max):
    dev, host = instance_pair(stress, device_bvh_opt=1, leaf_max=leaf_max)
    try:
        commit((dev, host), *motion(stress.arrays, 2))
        assert dev.stats()["bvh_instances"] == non_empty(stress.arrays)
        check_frames(stress, dev, host, "leaf_max %d" % leaf_max)
        check_data(stress.arrays, dev, host, leaf_max=leaf_max)
    finally:
        close(dev, host)


def fresh_at(scene, options, step):
    """a context whose only commit is `step`"""
    d = new_device(options)
    d.upload_scene(scene.scene.view)
    d.set_transforms(*motion(scene.arrays, step))
    return d


def same_data(a, b, what):
    fa, fb = frame_data(a), frame_data(b)
    for k in ("nodes", "tri_geom", "tri_shade", "lights"):
        assert fa[k].tobytes() == fb[k].tobytes(), "%s: %s differs" % (what, k)
    assert bits(a.stats()["bvh_sah"]) == bits(b.stats()["bvh_sah"]), what


@pytest.mark.gpu
def test_history_independence(stress):
    options = {"device_bvh": 1, "device_bvh_opt": 1, "device_bvh_instances": 1}
    a = fresh_at(stress, options, 0)
    b = None
    try:
        first, sah0, topo_ms = frame_data(a), a.stats()["bvh_sah"], a.stats()["bvh_topology_ms"]
        assert topo_ms > 0
        for k in range(1, 7):
            a.set_transforms(*motion(stress.arrays, k))
            assert a.stats()["bvh_topology_ms"] == topo_ms, "commit %d built the topology again" % k
        b = fresh_at(stress, options, 6)
        same_data(a, b, "steps 0..6 against step 6 alone")
        a.set_transforms(*motion(stress.arrays, 0))
        again = frame_data(a)
        assert again["nodes"].tobytes() == first["nodes"].tobytes() and again["tri_geom"].tobytes() == first["tri_geom"].tobytes()
        assert bits(a.stats()["bvh_sah"]) == bits(sah0) and a.stats()["bvh_topology_ms"] == topo_ms
    finally:
        close(*[d for d in (a, b) if d is not None])


@pytest.mark.gpu
def test_what_rebuilds_the_topology(cornell):
    s = cornell
    options = {"device_bvh": 1, "device_bvh_instances": 1, "device_bvh_refit": 8}
    dev, host = new_device(options), new_device(HOST)
    step = [0]
    k = non_empty(s.arrays)

    def advance(what, leaf_max=2, instances=k):
        """the next step on both contexts: exact frames, valid data, and the bytes of a context that has seen nothing else"""
        step[0] += 1
        commit((dev, host), *motion(s.arrays, step[0]))
        st = dev.stats()
        assert st["bvh_instances"] == instances and st["bvh_refits"] == 0 and st["bvh_builder"] == 1, (what, st)
        check_frames(s, dev, host, what)
        check_data(s.arrays, dev, host, leaf_max=leaf_max, partition=instances > 0)
        other = fresh_at(s, options, step[0])
        try:
            same_data(dev, other, what)
        finally:
            other.close()

    try:
        for d in (dev, host):
            d.upload_scene(s.scene.view)
        advance("first commit")
        advance("refits are ignored with the option on")
        options["leaf_max"] = 4
        dev.set_option("leaf_max", 4)
        host.set_option("leaf_max", 4)
        advance("leaf_max changed", leaf_max=4)
        options["device_bvh_opt"] = 1
        dev.set_option("device_bvh_opt", 1)
        advance("device_bvh_opt changed", leaf_max=4)
        for d in (dev, host):
            d.upload_scene(s.scene.view)
        advance("second hjr_upload_scene", leaf_max=4)
        options["device_bvh_instances"] = 0
        options["device_bvh_refit"] = 0
        dev.set_option("device_bvh_instances", 0)
        dev.set_option("device_bvh_refit", 0)
        advance("option off: an ordinary build", leaf_max=4, instances=0)
        options["device_bvh_instances"] = 1
        dev.set_option("device_bvh_instances", 1)
        dev.set_option("device_bvh_refit", 8)
        options["device_bvh_refit"] = 8
        advance("option on again", leaf_max=4)
        advance("and the commit after it", leaf_max=4)
    finally:
        close(dev, host)


def run_arrays(a, scene, options, integrator=hjr.INTEGRATOR_MIS):
    d = new_device(options)
    try:
        d.upload_arrays(a)
        d.set_transforms(a["transforms"], a["inv_transforms"])
        out = d.render(scene.hjr_params(64, 48, 4, integrator=integrator))
        return out, d.stats(), frame_data(d)
    finally:
        d.close()


def check_arrays(a, scene, what, instances=None, partition=True, opt=1):
    """the scene `a` under the option against the host build: frames, structure, instance count; returns the device's frame data"""
    (dc, da, dn), sd, fd = run_arrays(a, scene, {"device_bvh": 1, "device_bvh_opt": opt, "device_bvh_instances": 1})
    (hc, ha, hn), sh, fh = run_arrays(a, scene, HOST)
    for x, y, aov in ((dc, hc, "colour"), (da, ha, "albedo"), (dn, hn, "normal")):
        assert_bitexact(x, y, "%s (%s)" % (what, aov))
    assert sd["bvh_builder"] == 1 and sd["bvh_refits"] == 0
    assert sd["bvh_instances"] == (non_empty(a) if instances is None else instances), (what, sd["bvh_instances"])
    n = n_tris_of(a)
    validate_bvh4(fd, n, 2, sd["stack_need"])
    assert fd["tri_shade"].tobytes() == fh["tri_shade"].tobytes() and fd["lights"].tobytes() == fh["lights"].tobytes()
    if partition and sd["bvh_instances"]:
        check_partition(a, fd)
    return fd


def instance_tris(arrays, i):
    po = list(np.asarray(arrays["prim_offsets"], dtype=np.int64)) + [n_tris_of(arrays)]
    return list(range(int(po[i]), int(po[i + 1])))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["one instance", "two instances", "one-triangle instance", "empty instances", "same place"])
def test_shapes(cornell, shape):
    arrays = cornell.arrays
    sizes = instance_sizes(arrays)
    light_inst = int(prim_instance(arrays, arrays["light_prim_ids"][:1])[0])
    big = [int(i) for i in np.argsort(-sizes) if int(i) != light_inst]
    scene = cornell
    if shape == "one instance":
        a = sub_scene(arrays, instance_tris(arrays, light_inst))
        assert non_empty(a) == 1 and instance_sizes(a).size == sizes.size
    elif shape == "two instances":
        a = sub_scene(arrays, instance_tris(arrays, light_inst) + instance_tris(arrays, big[0]))
        assert non_empty(a) == 2
    elif shape == "one-triangle instance":
        a = sub_scene(arrays, instance_tris(arrays, light_inst) + instance_tris(arrays, big[0]) + instance_tris(arrays, big[1])[:1])
        assert 1 in instance_sizes(a).tolist() and non_empty(a) == 3
    elif shape == "empty instances":  # rotated, non-uniformly scaled and mirrored emitter instances, an empty one between them
        scene = TableScene(empty_before=True)
        a = scene.arrays
        assert 0 in instance_sizes(a).tolist() and non_empty(a) == scene.info["n_instances"] - 1
    else:
        a = same_place_scene(arrays, copies=64)
    fd = check_arrays(a, scene, shape)
    if shape == "same place":  # all boxes equal: the tie rule alone decides, the same way every run
        assert check_arrays(a, scene, shape + ", again")["nodes"].tobytes() == fd["nodes"].tobytes()


def placed(a, pre):
    """`a` with the 4 x 4 matrix pre[i] applied in front of instance i's transform; inverses in float64, cast"""
    m0 = np.asarray(a["transforms"], dtype=np.float64).reshape(-1, 3, 4)
    m, inv = np.zeros((m0.shape[0], 12), np.float32), np.zeros((m0.shape[0], 12), np.float32)
    for i in range(m0.shape[0]):
        full = pre[i] @ np.vstack([m0[i], [0, 0, 0, 1]])
        m[i] = full[:3].reshape(-1).astype(np.float32)
        inv[i] = np.linalg.inv(full)[:3].reshape(-1).astype(np.float32)
    out = dict(a)
    out["transforms"], out["inv_transforms"] = m, inv
    return out


def spread_scene(arrays, copies):
    """`copies` single-triangle instances on a 32-wide grid of small offsets"""
    pre = []
    for i in range(copies):
        t = np.eye(4)
        t[:3, 3] = [0.02 * ((i % 32) - 16), -0.01 * (i // 32), 0.02 * ((i // 32) - 16)]
        pre.append(t)
    return placed(same_place_scene(arrays, copies=copies), pre)


def nest_scene(arrays, copies=600):
    """`copies` instances of one triangle scaled about its world centroid by 1 + i / 100: every box encloses the ones before it, and
    the top tree is a chain"""
    a = same_place_scene(arrays, copies=copies)
    m0 = np.asarray(a["transforms"], dtype=np.float64).reshape(-1, 3, 4)[0]
    v = np.asarray(a["vertices"], dtype=np.float64).reshape(-1, 3)[np.asarray(a["indices"]).reshape(-1, 3)[0]]
    c = (v @ m0[:, :3].T + m0[:, 3]).mean(0)
    pre = []
    for i in range(copies):
        s = 1.0 + i / 100.0
        t = np.eye(4)
        t[:3, :3] *= s
        t[:3, 3] = c - s * c
        pre.append(t)
    return placed(a, pre)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["1024 instances", "1025 instances", "nest"])
def test_fallbacks(cornell, case):
    """At most HJR_TOP_MAX instances take the instance path; more of them, or a top tree deeper than the traversal stack, silently take
    the ordinary build.  Frames are exact either way."""
    if case == "nest":
        a, expect = nest_scene(cornell.arrays), 0
    else:
        copies = TOP_MAX if case.startswith("1024") else TOP_MAX + 1
        a, expect = spread_scene(cornell.arrays, copies), (TOP_MAX if case.startswith("1024") else 0)
    check_arrays(a, cornell, case, instances=expect, partition=False)


_batch = {}


@pytest.mark.gpu
@pytest.mark.parametrize("path_name", ["standalone", "fused"])
def test_rays_against_brute_force(stress, path_name):
    """the adversarial ray classes of tests/trace_util.py on the instance tree of step 3, bit for bit against the oracle's brute force"""
    if "b" not in _batch:
        a = dict(stress.arrays)
        a["transforms"], a["inv_transforms"] = motion(stress.arrays, 3)
        b = tu.Batch(a)
        b.ref  # noqa: B018
        _batch["a"], _batch["b"] = a, b
    a, b = _batch["a"], _batch["b"]
    path = {"standalone": hjr.TRACE_STANDALONE, "fused": hjr.TRACE_FUSED}[path_name]
    dev = stress.device({"device_bvh": 1, "device_bvh_opt": 1, "device_bvh_instances": 1})
    try:
        dev.set_transforms(a["transforms"], a["inv_transforms"])
        assert dev.stats()["bvh_instances"] == non_empty(stress.arrays)
        got = dev.trace_rays(path, b.shadow, b.closest)
        assert (got["status"] == hjr.TRACE_STATUS_OK).all()
        bad = tu.mismatches(got, b.ref)
        assert bad.size == 0, "%d of %d pairs differ from the brute force; first: %s" % (bad.size, got.size, [(int(i), got[i], b.ref[i]) for i in bad[:4]])
    finally:
        dev.close()


@pytest.mark.gpu
def test_tree_cost_against_refitting_forever(stress):
    """At step 15 of the motion the instance tree must cost less than the tree of a context that has refitted since step 0: both values
    come from this run, the second from the refit feature.  The ratio to a fresh ordinary build is printed, not asserted: an
    instance-partitioned tree cannot interleave overlapping instances."""
    base = {"device_bvh": 1, "device_bvh_opt": 1}
    inst = fresh_at(stress, dict(base, device_bvh_instances=1), 0)
    refit = fresh_at(stress, dict(base, device_bvh_refit=1000, device_bvh_refit_growth=10000), 0)
    full = fresh_at(stress, base, 0)
    try:
        for k in range(16):
            m, inv = motion(stress.arrays, k)
            if k > 0:
                refit.set_transforms(m, inv)
            if k in (7, 15):
                commit((inst, full), m, inv)
            if k in (0, 7, 15):
                si, sr, sf = inst.stats()["bvh_sah"], refit.stats()["bvh_sah"], full.stats()["bvh_sah"]
                print("step %2d: bvh_sah instance tree %.6g, refitted since step 0 %.6g, fresh ordinary build %.6g (instance / fresh %.3f)"
                      % (k, si, sr, sf, si / sf))
        assert refit.stats()["bvh_refits"] == 15 and inst.stats()["bvh_instances"] == non_empty(stress.arrays)
        assert si < sr, (si, sr)
    finally:
        close(inst, refit, full)


@pytest.mark.gpu
def test_cli_same_pngs(tmp_path):
    cli = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
    pngs, errs = [], []
    for flag in (False, True):
        work = tmp_path / ("run%d" % flag)
        shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
        ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
        ro["Image"].update(image_width=96, image_height=64, max_spp=8, image_name="inst")
        ro["Animation"].update(start_frame=1, end_frame=3)
        ro["Henjou_HIP"] = {"seed": 5, "device_bvh": True, "device_bvh_opt": 1, "force_rebuild": True, "verbose": True}
        if flag:
            ro["Henjou_HIP"]["device_bvh_instances"] = True
        (work / "render_option.json").write_text(json.dumps(ro))
        (work / "fps.txt").write_text("24")
        p = subprocess.run([cli, "render_option.json"], cwd=work, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        pngs.append([(work / ("inst_%03d.png" % f)).read_bytes() for f in (1, 2)])
        errs.append([ln for ln in p.stderr.splitlines() if "device build" in ln or "device instance build" in ln])
    assert pngs[0] == pngs[1]
    assert errs[0] and not any("instance build" in ln for ln in errs[0]), errs[0]
    assert errs[1] and all("device instance build" in ln for ln in errs[1]), errs[1]
