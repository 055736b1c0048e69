"""Option "device_bvh_graft" (with "device_bvh" 1 and "device_bvh_instances" 1): every instance's BVH4 is collapsed once per topology from
the object-space boxes (the skeleton) and grafted under a BVH4 top tree that every commit builds over the instances' world boxes
(csrc/hjr_bvh_build.hip).  Frames do not depend on the tree, so every frame must be the host-built context's bits.  The
frame data is checked through hjr_copy_frame_data like that of the instance trees: a valid BVH4 with tight padded boxes, the host's
records, instances as whole subtrees; and on top of it the skeleton's refs rows must not change between commits.

The nodes are not the bytes of "device_bvh_instances" 1 alone (that mode collapses with world-space areas and lets a top node absorb an
instance root's children), so nothing here compares against it except the printed cost ratios.
"""
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
from test_device_bvh_refit import motion, split_nodes, tight_boxes, check_frames
from test_device_bvh_instances import (HOST, TOP_MAX, LEAF_FLAG, _option_json, bits, check_data, check_partition, close, commit, instance_sizes,
                                       instance_tris, n_tris_of, nest_scene, non_empty, prim_instance, same_data, spread_scene)
from test_gpu_parity import assert_bitexact

GRAFT = {"device_bvh": 1, "device_bvh_instances": 1, "device_bvh_graft": 1}


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_render_option_parses_device_bvh_graft(tmp_path):
    """"device_bvh_graft": true is bit 9 of hjr_render_option.device_bvh_opt, next to bit 8 ("device_bvh_instances") and the rounds in the
    low 8 bits; the refusals name the key."""
    load = lambda extra: hjr.load_render_option(_option_json(tmp_path, extra))  # noqa: E731
    on = {"device_bvh": True, "device_bvh_instances": True}
    assert load(dict(on, device_bvh_graft=True)).device_bvh_opt == 0x300
    assert load(dict(on, device_bvh_graft=1, device_bvh_opt=2)).device_bvh_opt == 0x302
    assert load(dict(on, device_bvh_graft=False, device_bvh_opt=3)).device_bvh_opt == 0x103
    assert load(dict(on, device_bvh_graft=0)).device_bvh_opt == 0x100
    assert load(dict(on, device_bvh_opt=1)).device_bvh_opt == 0x101
    o = load(dict(on, device_bvh_graft=True, device_bvh_refit=8))
    assert o.device_bvh == 9 and o.device_bvh_opt == 0x300
    for bad in ({"device_bvh_graft": True}, {"device_bvh": True, "device_bvh_graft": True},
                {"device_bvh": True, "device_bvh_instances": False, "device_bvh_graft": True}, {"device_bvh": True, "device_bvh_instances": False, "device_bvh_graft": False},
                dict(on, device_bvh_graft="yes"), dict(on, device_bvh_graft=2), dict(on, device_bvh_graft=-1)):
        with pytest.raises(hjr.HjrError, match="device_bvh_graft"):
            load(bad)


# ---------------------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def stress(tmp_path_factory):
    s = StressScene(tmp_path_factory.mktemp("graft"), spheres=8, segments=32)
    assert s.scene.view.n_triangles > 4 * 256 * 4 and non_empty(s.arrays) >= 8  # several workgroups of skeleton nodes
    return s


@pytest.fixture(scope="module")
def scenes(cornell, stress):
    return {"cornell": cornell, "stress": stress}


def graft_pair(scene, **opts):
    return host_device_pair(scene, device_bvh_instances=1, device_bvh_graft=1, **opts)


def fresh_at(scene, options, step):
    """a context whose only commit is `step`"""
    d = new_device(options)
    d.upload_scene(scene.scene.view)
    d.set_transforms(*motion(scene.arrays, step))
    return d


def top_nodes(arrays, fd):
    """Which nodes belong to the top tree: those with whole instances of more than one id below them.  (A node of the skeleton has
    triangles of one instance only; a top node always joins at least two, also when each of its slots holds a single one.)  Returns the
    flags; the top nodes must be the ids [0, base)."""
    sizes = instance_sizes(arrays)
    row_inst = prim_instance(arrays, fd["tri_geom"].reshape(-1, 12)[:, 9].view(np.uint32))
    refs, _, _ = split_nodes(fd)
    n_nodes, n_inst = refs.shape[0], sizes.size
    below = np.zeros((n_nodes, n_inst), dtype=np.int64)  # triangles of each instance below each node (check_partition's `below`, summed over the slots)
    for i in range(n_nodes - 1, -1, -1):
        for s in range(4):
            r = int(refs[i, s])
            if r == LEAF_FLAG:
                continue
            if r & LEAF_FLAG:
                f, c = r & 0x7FFFFFF, (r >> 27) & 15
                below[i] += np.bincount(row_inst[f:f + c], minlength=n_inst)
            else:
                below[i] += below[r]
    touched = below > 0
    assert np.all(~touched | (touched.sum(-1, keepdims=True) == 1) | (below == sizes)), "a node cuts through an instance while holding another one"
    top = touched.sum(-1) > 1
    base = int(top.sum())
    assert np.all(top[:base]) and not np.any(top[base:]), "the top nodes are not the first ids"
    return top


def skeleton_rows(arrays, fd):
    """(base, refs rows of the skeleton with base subtracted from the inner refs)"""
    top = top_nodes(arrays, fd)
    base = int(top.sum())
    refs = split_nodes(fd)[0][base:].astype(np.int64)
    inner = (refs & LEAF_FLAG) == 0
    assert np.all(refs[inner] >= base)
    refs[inner] -= base
    return base, refs.astype(np.uint32)


@pytest.mark.gpu
def test_option_round_trip_and_inert_without_instance_trees(cornell):
    d = new_device()
    try:
        assert d.get_option("device_bvh_graft") == -1
        for v in (0, 1):
            d.set_option("device_bvh_graft", v)
            assert d.get_option("device_bvh_graft") == v
        for bad in (2, -2):
            with pytest.raises(hjr.HjrError):
                d.set_option("device_bvh_graft", bad)
    finally:
        d.close()
    m, inv = motion(cornell.arrays, 2)
    for name, with_it, without in (("device_bvh 0", dict(HOST, device_bvh_instances=1, device_bvh_graft=1), dict(HOST, device_bvh_instances=1)),
                                   ("device_bvh_instances 0", {"device_bvh": 1, "device_bvh_opt": 1, "device_bvh_graft": 1}, {"device_bvh": 1, "device_bvh_opt": 1})):
        a, b = cornell.device(with_it), cornell.device(without)
        try:
            commit((a, b), m, inv)
            sa, sb = a.stats(), b.stats()
            assert sa["bvh_instances"] == 0 and sa["bvh_topology_ms"] == 0.0 and sa["bvh_builder"] == sb["bvh_builder"], (name, sa)
            assert sa["bvh_nodes"] == sb["bvh_nodes"] and bits(sa["bvh_sah"]) == bits(sb["bvh_sah"]) and sa["stack_need"] == sb["stack_need"], name
            fa, fb = frame_data(a), frame_data(b)
            for k in fa:
                assert fa[k].tobytes() == fb[k].tobytes(), (name, k)
        finally:
            close(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", [0, 1])
@pytest.mark.parametrize("name", ["cornell", "stress"])
def test_animated_frames_frame_data_and_fixed_skeleton(scenes, name, opt):
    s = scenes[name]
    dev, host = graft_pair(s, device_bvh_opt=opt)
    try:
        prims = rows = skel_nodes = topo_ms = None
        for k in range(6):
            commit((dev, host), *motion(s.arrays, k))
            st = dev.stats()
            assert st["bvh_instances"] == non_empty(s.arrays) and st["bvh_refits"] == 0 and st["bvh_builder"] == 1, (k, st)
            check_frames(s, dev, host, "%s, opt %d, step %d" % (name, opt, k))
            if k == 2:
                check_frames(s, dev, host, "%s, step %d, MIS" % (name, k), integrator=hjr.INTEGRATOR_MIS)
            if k == 4:
                check_frames(s, dev, host, "%s, step %d, Pathtrace" % (name, k), integrator=hjr.INTEGRATOR_PT)
            fd = check_data(s.arrays, dev, host)  # validate_bvh4, tight boxes, the host's records, check_partition, bvh_sah against sah64
            col = fd["tri_geom"].reshape(-1, 12)[:, 9].tobytes()
            assert prims is None or col == prims, "the leaf order changed at step %d" % k
            prims = col
            p = s.hjr_params(64, 48, 1)
            assert dev.gbuffer(p).tobytes() == host.gbuffer(p).tobytes(), "G-buffer (tri_inst) differs at step %d" % k
            # the skeleton is fixed: only the top nodes and the boxes change between commits
            base, r = skeleton_rows(s.arrays, fd)
            assert base >= 1 and st["bvh_nodes"] == split_nodes(fd)[0].shape[0]
            if rows is None:
                rows, skel_nodes, topo_ms = r.tobytes(), st["bvh_nodes"] - base, st["bvh_topology_ms"]
                assert topo_ms > 0
            assert r.tobytes() == rows, "the skeleton's refs rows changed at step %d" % k
            assert st["bvh_nodes"] - base == skel_nodes, (k, st["bvh_nodes"], base, skel_nodes)
            assert st["bvh_topology_ms"] == topo_ms, "commit %d built the topology again" % k
    finally:
        close(dev, host)


@pytest.mark.gpu
@pytest.mark.parametrize("leaf_max", [1, 4])
def test_leaf_max(stress, leaf_max):
    dev, host = graft_pair(stress, device_bvh_opt=1, leaf_max=leaf_max)
    try:
        commit((dev, host), *motion(stress.arrays, 2))
        assert dev.stats()["bvh_instances"] == non_empty(stress.arrays)
        check_frames(stress, dev, host, "leaf_max %d" % leaf_max)
        check_data(stress.arrays, dev, host, leaf_max=leaf_max)
    finally:
        close(dev, host)


@pytest.mark.gpu
def test_history_independence(stress):
    options = dict(GRAFT, device_bvh_opt=1)
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
def test_what_rebuilds_the_skeleton(cornell):
    s = cornell
    options = dict(GRAFT, device_bvh_refit=8)
    dev, host = new_device(options), new_device(HOST)
    step = [0]
    k = non_empty(s.arrays)
    seen = []

    def advance(what, leaf_max=2, instances=k):
        """the next step on both contexts: exact frames, valid data, and the bytes of a context that has seen nothing else"""
        step[0] += 1
        commit((dev, host), *motion(s.arrays, step[0]))
        st = dev.stats()
        assert st["bvh_instances"] == instances and st["bvh_refits"] == 0 and st["bvh_builder"] == 1, (what, st)
        check_frames(s, dev, host, what)
        fd = check_data(s.arrays, dev, host, leaf_max=leaf_max, partition=instances > 0)
        other = fresh_at(s, options, step[0])
        try:
            same_data(dev, other, what)
        finally:
            other.close()
        seen.append((what, st["bvh_topology_ms"], skeleton_rows(s.arrays, fd)[1].tobytes() if instances else None))

    try:
        for d in (dev, host):
            d.upload_scene(s.scene.view)
        advance("first commit")
        advance("refits are ignored with the option on")
        assert seen[1][1] == seen[0][1] and seen[1][2] == seen[0][2], "the second commit built the skeleton again"
        options["leaf_max"] = 4
        dev.set_option("leaf_max", 4)
        host.set_option("leaf_max", 4)
        advance("leaf_max changed", leaf_max=4)
        assert seen[2][2] != seen[1][2], "leaf_max 4 left the skeleton of leaf_max 2"
        options["device_bvh_opt"] = 1
        dev.set_option("device_bvh_opt", 1)
        advance("device_bvh_opt changed", leaf_max=4)
        for d in (dev, host):
            d.upload_scene(s.scene.view)
        advance("second hjr_upload_scene", leaf_max=4)
        options["device_bvh_graft"] = 0
        dev.set_option("device_bvh_graft", 0)
        advance("option off: instance trees alone", leaf_max=4)
        options["device_bvh_graft"] = 1
        dev.set_option("device_bvh_graft", 1)
        advance("option on again", leaf_max=4)
        advance("and the commit after it", leaf_max=4)
        assert seen[-1][1] == seen[-2][1] and seen[-1][2] == seen[-2][2] == seen[4][2]
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


def check_arrays(a, scene, what, instances=None, partition=True, opt=1, leaf_max=2):
    """the scene `a` under the option against the host build: frames, structure, instance count; returns (stats, frame data)"""
    (dc, da, dn), sd, fd = run_arrays(a, scene, dict(GRAFT, device_bvh_opt=opt, leaf_max=leaf_max))
    (hc, ha, hn), sh, fh = run_arrays(a, scene, dict(HOST, leaf_max=leaf_max))
    for x, y, aov in ((dc, hc, "colour"), (da, ha, "albedo"), (dn, hn, "normal")):
        assert_bitexact(x, y, "%s (%s)" % (what, aov))
    assert sd["bvh_builder"] == 1 and sd["bvh_refits"] == 0
    assert sd["bvh_instances"] == (non_empty(a) if instances is None else instances), (what, sd["bvh_instances"])
    validate_bvh4(fd, n_tris_of(a), leaf_max, sd["stack_need"])
    assert fd["tri_shade"].tobytes() == fh["tri_shade"].tobytes() and fd["lights"].tobytes() == fh["lights"].tobytes()
    if partition and sd["bvh_instances"]:
        check_partition(a, fd)
    return sd, fd


def with_empty_instances(arrays):
    """`arrays` with an instance without triangles (and the transform of a neighbour) first, after the second instance and last"""
    po = np.asarray(arrays["prim_offsets"], dtype=np.uint32).reshape(-1)
    n, k = n_tris_of(arrays), po.size
    src = [0] + [0, 1] + [1] + list(range(2, k)) + [k - 1]          # the instance each new one copies its transform from
    off = [0] + [po[0], po[1]] + [po[2] if k > 2 else n] + [po[i] for i in range(2, k)] + [n]
    a = dict(arrays)
    a["prim_offsets"] = np.array(off, dtype=np.uint32)
    for key in ("transforms", "inv_transforms"):
        a[key] = np.asarray(arrays[key], dtype=np.float32).reshape(-1, 12)[src].copy()
    return a


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
    elif shape == "empty instances":  # empty instances first, last and in between
        a = with_empty_instances(arrays)
        es = instance_sizes(a).tolist()
        assert es[0] == 0 and es[-1] == 0 and es[3] == 0 and non_empty(a) == sizes.size and sum(es) == n_tris_of(arrays)
    else:
        a = same_place_scene(arrays, copies=64)
    sd, fd = check_arrays(a, scene, shape)
    base = int(top_nodes(a, fd).sum())
    if shape == "one instance":
        # at most leaf_max triangles: the one-leaf root; with leaf_max 1 the same instance has a node, and its skeleton is the tree
        assert sizes[light_inst] == 2 and sd["bvh_nodes"] == 1 and int((split_nodes(fd)[0] != LEAF_FLAG).sum()) == 1
        sd1, fd1 = check_arrays(a, scene, shape + ", leaf_max 1", leaf_max=1)
        assert sd1["bvh_nodes"] == 1 and int((split_nodes(fd1)[0] != LEAF_FLAG).sum()) == 2
        whole = dict(arrays, prim_offsets=np.zeros_like(arrays["prim_offsets"]))  # ... and the whole scene as the last instance: base 0
        assert non_empty(whole) == 1
        sd2, fd2 = check_arrays(whole, scene, shape + ", the whole scene")
        assert int(top_nodes(whole, fd2).sum()) == 0 and sd2["bvh_nodes"] > 256
    if shape == "one-triangle instance":  # a leaf slot of one triangle in a top node
        refs = split_nodes(fd)[0][:base]
        one = prim_instance(a, fd["tri_geom"].reshape(-1, 12)[:, 9].view(np.uint32)) == int(np.nonzero(instance_sizes(a) == 1)[0][0])
        assert (LEAF_FLAG | (1 << 27) | int(np.nonzero(one)[0][0])) in refs.reshape(-1).tolist()
    if shape == "same place":  # all boxes equal: the tie rule alone decides, the same way every run
        assert base == sd["bvh_nodes"]  # one-triangle instances have no nodes of their own
        assert check_arrays(a, scene, shape + ", again")[1]["nodes"].tobytes() == fd["nodes"].tobytes()


@pytest.mark.gpu
def test_scaled_and_mirrored_instances():
    """Rotated, non-uniformly scaled and mirrored instances: the areas that order the skeleton's slots (object space) and those of the
    boxes it carries (world space) disagree, which may cost traversal steps and never a hit."""
    for kw in (dict(), dict(empty_before=True)):
        scene = TableScene(**kw)
        a = scene.arrays
        m = np.asarray(a["transforms"], dtype=np.float64).reshape(-1, 3, 4)[:, :, :3]
        sv = np.linalg.svd(m, compute_uv=False)
        assert np.any(np.linalg.det(m) < 0) and np.any(sv[:, 0] / sv[:, 2] > 1.5)  # mirrored ones and non-uniform scales are there
        for opt in (0, 1):
            sd, fd = check_arrays(a, scene, "table scene %s, opt %d" % (kw, opt), opt=opt)
            check_data_boxes(fd)


def check_data_boxes(fd):
    refs, lo, hi = split_nodes(fd)
    elo, ehi = tight_boxes(fd)
    used = refs != LEAF_FLAG
    assert lo[used].tobytes() == elo[used].tobytes() and hi[used].tobytes() == ehi[used].tobytes(), "slot boxes are not the tight padded boxes"


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["1024 instances", "1025 instances", "nest"])
def test_fallbacks(cornell, case):
    """At most HJR_TOP_MAX instances take the graft path; more of them, or a top tree deeper than the traversal stack, silently take the
    ordinary build.  Frames are exact either way."""
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
    """the adversarial ray classes of tests/trace_util.py on the grafted tree of step 3, bit for bit against the oracle's brute force"""
    if "b" not in _batch:
        a = dict(stress.arrays)
        a["transforms"], a["inv_transforms"] = motion(stress.arrays, 3)
        b = tu.Batch(a)
        b.ref  # noqa: B018
        _batch["a"], _batch["b"] = a, b
    a, b = _batch["a"], _batch["b"]
    path = {"standalone": hjr.TRACE_STANDALONE, "fused": hjr.TRACE_FUSED}[path_name]
    dev = stress.device(dict(GRAFT, device_bvh_opt=1))
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
    """At step 15 of the motion the grafted tree must cost less than the tree of a context that has refitted since step 0: both values
    come from this run.  The ratios to "device_bvh_instances" 1 alone and to a fresh ordinary build are printed, not asserted."""
    base = {"device_bvh": 1, "device_bvh_opt": 1}
    graft = fresh_at(stress, dict(base, device_bvh_instances=1, device_bvh_graft=1), 0)
    inst = fresh_at(stress, dict(base, device_bvh_instances=1), 0)
    refit = fresh_at(stress, dict(base, device_bvh_refit=1000, device_bvh_refit_growth=10000), 0)
    full = fresh_at(stress, base, 0)
    try:
        for k in range(16):
            m, inv = motion(stress.arrays, k)
            if k > 0:
                refit.set_transforms(m, inv)
            if k in (7, 15):
                commit((graft, inst, full), m, inv)
            if k in (0, 7, 15):
                sg, si, sr, sf = (d.stats()["bvh_sah"] for d in (graft, inst, refit, full))
                print("step %2d: bvh_sah grafted %.6g, refitted since step 0 %.6g, instance trees alone %.6g (grafted / alone %.3f), fresh ordinary build "
                      "%.6g (grafted / fresh %.3f)" % (k, sg, sr, si, sg / si, sf, sg / sf))
        assert refit.stats()["bvh_refits"] == 15 and graft.stats()["bvh_instances"] == non_empty(stress.arrays)
        assert sg < sr, (sg, sr)
    finally:
        close(graft, inst, refit, full)


@pytest.mark.gpu
def test_cli_same_pngs(tmp_path):
    cli = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
    pngs, errs = [], []
    for flag in (False, True):
        work = tmp_path / ("run%d" % flag)
        shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
        ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
        ro["Image"].update(image_width=96, image_height=64, max_spp=8, image_name="graft")
        ro["Animation"].update(start_frame=1, end_frame=3)
        ro["Henjou_HIP"] = {"seed": 5, "device_bvh": True, "device_bvh_opt": 1, "device_bvh_instances": True, "force_rebuild": True, "verbose": True}
        if flag:
            ro["Henjou_HIP"]["device_bvh_graft"] = True
        (work / "render_option.json").write_text(json.dumps(ro))
        (work / "fps.txt").write_text("24")
        p = subprocess.run([cli, "render_option.json"], cwd=work, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        pngs.append([(work / ("graft_%03d.png" % f)).read_bytes() for f in (1, 2)])
        errs.append([ln for ln in p.stderr.splitlines() if "instance build" in ln])
    assert pngs[0] == pngs[1]
    assert errs[0] and not any("grafted" in ln for ln in errs[0]), errs[0]
    assert errs[1] and all("device grafted instance build" in ln for ln in errs[1]), errs[1]
