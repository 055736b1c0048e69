"""Deforming meshes on the GPU: hjr_update_vertices, hjr_set_morph, hjr_set_morph_weights (include/henjou_hip.h).

Frames depend on the triangles, not on the tree, so every deformed frame is checked bit for bit against the unchanged oracle, fed the
numpy-blended arrays (tests/deform_util.py) as a static scene: "equals the static upload" = the three AOVs are the oracle's bits, the ray,
hit and light-sample counters are the oracle's, and the oracle's deformed frame differs from its base frame in at least 1/16 of the pixels
(asserted on the oracle's frames alone, so a case cannot be vacuous).  32 x 32 at 8 spp (16 where a frame is rendered in two passes).
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import deform_util as du
import oracle_binding as ob
from scene_util import Cornell, hjr, f32_time, new_device

pytestmark = pytest.mark.gpu

W, H, SPP = 32, 32, 8
NEE, MIS = hjr.INTEGRATOR_NEE, hjr.INTEGRATOR_MIS
COUNTERS = ("samples", "closest_rays", "shadow_rays", "shaded_hits", "light_samples", "nan_samples")
ERR_ARG, ERR_STATE = -1, -5


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def std(cornell):
    return du.standard_sets(cornell.arrays)


_frames = {}


def oracle_frame(cornell, arrays, integrator=NEE, spp=SPP):
    """(colour, albedo, normal, stats) of the oracle on `arrays` as a static scene; one render per distinct geometry and integrator"""
    k = (np.asarray(arrays["vertices"]).tobytes(), np.asarray(arrays["normals"]).tobytes(), integrator, spp)
    if k not in _frames:
        _frames[k] = ob.OracleScene(arrays, ob.MATH_PORTABLE).render(cornell.oracle_params(W, H, spp, integrator=integrator))
    return _frames[k]


def bits_equal(a, b, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    same = a.view(np.uint32) == b.view(np.uint32)
    assert same.all(), "%s: %d of %d values differ" % (what, int((~same).sum()), same.size)


def equals_static_upload(cornell, dev, arrays, what, integrator=NEE, spp=SPP, vacuity=True):
    oc, oa, on, ost = oracle_frame(cornell, arrays, integrator, spp)
    if vacuity:
        frac = du.changed_fraction(oc, oracle_frame(cornell, cornell.arrays, integrator, spp)[0])
        assert frac >= 1.0 / 16.0, "%s: the oracle's deformed frame differs from its base frame in %.3f of the pixels only" % (what, frac)
    c, a, n = dev.render(cornell.hjr_params(W, H, spp, integrator=integrator, flags=hjr.FLAG_STATS))
    st = dev.stats()
    bits_equal(c, oc, what + ", colour")
    bits_equal(a, oa, what + ", albedo")
    bits_equal(n, on, what + ", normal")
    for k in COUNTERS:
        assert st[k] == ost[k], (what, k, st[k], ost[k])
    return st


def xf(cornell):
    return cornell.arrays["transforms"], cornell.arrays["inv_transforms"]


# ---------------------------------------------------------------------------------------------------------------- 1. morph, then render
@pytest.mark.parametrize("integrator", [NEE, MIS], ids=["nee", "mis"])
@pytest.mark.parametrize("pipeline", [1, 2], ids=["mega", "wf"])
@pytest.mark.parametrize("device_bvh", [0, 1], ids=["host", "device"])
def test_morph_equals_the_static_upload(cornell, std, device_bvh, pipeline, integrator):
    sets, w = std
    blended = du.apply_morph(cornell.arrays, sets, w)
    d = cornell.device({"device_bvh": device_bvh, "pipeline": pipeline})
    try:
        g0 = d.stats()["geometry_generation"]
        d.set_morph(sets, w)
        d.set_transforms(*xf(cornell))  # unchanged transforms: not "unchanged" frame data
        st = equals_static_upload(cornell, d, blended, "morph, device_bvh %d" % device_bvh, integrator)
        assert st["pipeline"] == pipeline - 1 and st["bvh_builder"] == device_bvh
        assert st["morph_vertices"] == du.n_morph_vertices(sets) and st["geometry_generation"] > g0
        if device_bvh:
            fresh = hjr.Device(0)
            try:
                fresh.set_option("device_bvh", 1)
                fresh.upload_arrays(blended)
                fresh.set_transforms(*xf(cornell))
                assert fresh.stats()["morph_vertices"] == 0
                assert du.world_vertices_by_prim(d, hjr).tobytes() == du.world_vertices_by_prim(fresh, hjr).tobytes()
            finally:
                fresh.close()
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the light follows
@pytest.mark.parametrize("device_bvh", [0, 1], ids=["host", "device"])
def test_a_morphed_light_equals_the_static_upload(cornell, device_bvh):
    """One set over the light's vertices alone: the light table, its area and its pdf follow the deformation (in device mode the table is
    built on the host from the light triangles' vertices only)."""
    a = cornell.arrays
    l0, l1 = du.instance_vertex_range(a, du.light_instance(a))
    rng = np.random.default_rng(3)
    sets = [du.make_set(rng, l0, l1 - l0, 1, 0, 0.1 * du.scene_extent(a), True)]
    w = np.array([1.5], np.float32)
    blended = du.apply_morph(a, sets, w)
    d = cornell.device({"device_bvh": device_bvh})
    try:
        d.set_morph(sets, w)
        d.set_transforms(*xf(cornell))
        equals_static_upload(cornell, d, blended, "morphed light, device_bvh %d" % device_bvh)
        fresh = hjr.Device(0)
        try:
            fresh.set_option("device_bvh", device_bvh)
            fresh.upload_arrays(blended)
            fresh.set_transforms(*xf(cornell))
            rows, want = d.copy_frame_data(hjr.FRAME_LIGHTS), fresh.copy_frame_data(hjr.FRAME_LIGHTS)
            assert rows.tobytes() == want.tobytes(), "light table"
            assert rows.tobytes() != cornell.device().copy_frame_data(hjr.FRAME_LIGHTS).tobytes(), "the light table did not move"
        finally:
            fresh.close()
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------------------- 3. weight sequences
def test_weight_sequence_refits(cornell, std):
    sets, _ = std
    d = new_device({"device_bvh": 1, "device_bvh_refit": 8})
    try:
        d.upload_scene(cornell.scene.view)
        d.set_morph(sets, du.WEIGHT_SEQUENCE[0])  # ahead of the first commit: frame 0 is the full build
        for f, w in enumerate(du.WEIGHT_SEQUENCE):
            d.set_morph_weights(w)
            d.set_transforms(*xf(cornell))
            st = equals_static_upload(cornell, d, du.apply_morph(cornell.arrays, sets, w), "sequence frame %d" % f)
            assert st["bvh_refits"] == f, (f, st["bvh_refits"])
            assert st["morph_vertices"] == du.n_morph_vertices(sets)
        gen = st["geometry_generation"]
        d.set_morph_weights(du.WEIGHT_SEQUENCE[-1])  # the fourth's weights again: the frame data is reused
        d.set_transforms(*xf(cornell))
        st = d.stats()
        assert st["geometry_generation"] == gen and st["morph_vertices"] == 0 and st["bvh_refits"] == len(du.WEIGHT_SEQUENCE) - 1
        equals_static_upload(cornell, d, du.apply_morph(cornell.arrays, sets, du.WEIGHT_SEQUENCE[-1]), "fifth commit")
        # a forced commit with these weights builds again but has nothing to blend: the working arrays are current
        d.set_option("force_rebuild", 1)
        d.set_transforms(*xf(cornell))
        st = d.stats()
        assert st["morph_vertices"] == 0 and st["bvh_refits"] == len(du.WEIGHT_SEQUENCE)
        equals_static_upload(cornell, d, du.apply_morph(cornell.arrays, sets, du.WEIGHT_SEQUENCE[-1]), "forced commit, same weights")
    finally:
        d.close()


@pytest.mark.parametrize("graft", [0, 1], ids=["instances", "graft"])
def test_weight_sequence_with_instance_trees(cornell, std, graft):
    sets, _ = std
    d = cornell.device({"device_bvh": 1, "device_bvh_refit": 8, "device_bvh_instances": 1, "device_bvh_graft": graft})
    try:
        d.set_morph(sets, du.WEIGHT_SEQUENCE[0])
        for f, w in enumerate(du.WEIGHT_SEQUENCE):
            d.set_morph_weights(w)
            d.set_transforms(*xf(cornell))
            st = equals_static_upload(cornell, d, du.apply_morph(cornell.arrays, sets, w), "instance sequence frame %d, graft %d" % (f, graft))
            assert st["bvh_instances"] > 0 and st["bvh_refits"] == 0 and st["morph_vertices"] == du.n_morph_vertices(sets)
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------------------- 4. hjr_update_vertices
@pytest.mark.parametrize("device_bvh", [0, 1], ids=["host", "device"])
def test_update_vertices_then_morph(cornell, std, device_bvh):
    sets, w = std
    a = cornell.arrays
    rng = np.random.default_rng(5)
    first, cnt = 700, 1501  # a sub-range inside the large instance; it overlaps set B's neighbourhood but no set's base is special
    scale = 0.1 * du.scene_extent(a)
    d = cornell.device({"device_bvh": device_bvh})
    try:
        e1 = dict(a)
        v = np.array(a["vertices"], np.float32).reshape(-1, 3)
        v[first:first + cnt] += (rng.uniform(-1, 1, (cnt, 3)) * scale).astype(np.float32)
        e1["vertices"] = v.reshape(-1)
        d.update_vertices(first, v[first:first + cnt])  # normals NULL: kept
        d.set_transforms(*xf(cornell))
        equals_static_upload(cornell, d, e1, "update, positions only")
        e2 = dict(e1)
        v2 = v.copy()
        n2 = np.array(a["normals"], np.float32).reshape(-1, 3)
        f2, c2 = 36, 300
        v2[f2:f2 + c2] += (rng.uniform(-1, 1, (c2, 3)) * scale).astype(np.float32)
        n2[f2:f2 + c2] += rng.uniform(-0.3, 0.3, (c2, 3)).astype(np.float32)
        e2["vertices"], e2["normals"] = v2.reshape(-1), n2.reshape(-1)
        d.update_vertices(f2, v2[f2:f2 + c2], n2[f2:f2 + c2])
        d.set_transforms(*xf(cornell))
        st = equals_static_upload(cornell, d, e2, "update with normals")
        assert st["morph_vertices"] == 0
        d.set_morph(sets, w)  # on top of the edited base
        d.set_transforms(*xf(cornell))
        st = equals_static_upload(cornell, d, du.apply_morph(e2, sets, w), "morph over the edited base")
        assert st["morph_vertices"] == du.n_morph_vertices(sets)
        if device_bvh:  # the base changes under a morph whose working arrays are on the device
            d.update_vertices(first, np.array(a["vertices"], np.float32).reshape(-1, 3)[first:first + cnt])
            d.set_transforms(*xf(cornell))
            e3 = dict(e2)
            v3 = v2.copy()
            v3[first:first + cnt] = np.array(a["vertices"], np.float32).reshape(-1, 3)[first:first + cnt]
            e3["vertices"] = v3.reshape(-1)
            equals_static_upload(cornell, d, du.apply_morph(e3, sets, w), "base edited under the morph")
        d.set_morph(None)  # removed: the edited base
        d.set_transforms(*xf(cornell))
        assert d.stats()["morph_vertices"] == 0
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------------------- 5. state rules
def with_range(p, begin, end):
    q = hjr.ParamsV2.from_buffer_copy(p)
    q.sample_begin, q.sample_end = begin, end
    return q


def render_rc(dev, p):
    out = np.zeros((p.height, p.width, 4), np.float32)
    return hjr.lib().hjr_render(dev._h, C.byref(p), out.ctypes.data, None, None), out


def test_an_update_ends_an_open_progressive_frame(cornell, std):
    sets, w = std
    d = cornell.device()
    try:
        d.set_morph(sets, w)
        d.set_transforms(*xf(cornell))
        p = cornell.hjr_params(W, H, 16)
        v = np.array(cornell.arrays["vertices"], np.float32).reshape(-1, 3)
        for what, call in (("update_vertices", lambda: d.update_vertices(100, v[100:164])), ("set_morph_weights", lambda: d.set_morph_weights(w)),
                           ("set_morph", lambda: d.set_morph(sets, w))):
            rc, _ = render_rc(d, with_range(p, 0, 8))
            assert rc == 0, hjr.lib().hjr_last_error()
            call()
            rc, _ = render_rc(d, with_range(p, 8, 16))
            assert rc == ERR_STATE, (what, rc, hjr.lib().hjr_last_error())
        # and a frame started after the commit completes: its two passes give the one-shot frame of the static upload
        d.set_transforms(*xf(cornell))
        rc, _ = render_rc(d, with_range(p, 0, 8))
        assert rc == 0
        rc, out = render_rc(d, with_range(p, 8, 16))
        assert rc == 0
        bits_equal(out, oracle_frame(cornell, du.apply_morph(cornell.arrays, sets, w), NEE, 16)[0], "two passes over the morphed scene")
    finally:
        d.close()


def test_an_update_drops_the_temporal_history(cornell, std):
    sets, w = std
    mode = hjr.MODE_DENOISE
    p1, p2 = cornell.hjr_params(W, H, SPP, frame=1), cornell.hjr_params(W, H, SPP, frame=2)
    v = np.array(cornell.arrays["vertices"], np.float32).reshape(-1, 3)
    calls = {"update_vertices": lambda d: d.update_vertices(100, v[100:164] + np.float32(0.05)),
             "set_morph": lambda d: d.set_morph(sets, w), "set_morph_weights": lambda d: d.set_morph_weights(w * np.float32(0.5))}
    for what, call in calls.items():
        a, b = cornell.device(), cornell.device()
        try:
            for d in (a, b):
                d.set_option("denoise_temporal", 1)
                if what == "set_morph_weights":
                    d.set_morph(sets, w)
                    d.set_transforms(*xf(cornell))
            a.render_denoised(p1, mode)  # a history
            with_hist = a.render_denoised(p2, mode)
            a.temporal_reset()
            assert not np.array_equal(with_hist, a.render_denoised(p2, mode)), "the history has no effect: the case shows nothing"
            a.render_denoised(p1, mode)
            for d in (a, b):
                call(d)
                d.set_transforms(*xf(cornell))
            bits_equal(a.render_denoised(p2, mode), b.render_denoised(p2, mode), "frame after " + what)
        finally:
            a.close()
            b.close()


def test_argument_errors_change_nothing(cornell, std):
    sets, w = std
    nv = cornell.scene.view.n_vertices
    L = hjr.lib()
    d = cornell.device({"device_bvh": 1})
    try:
        d.set_morph(sets, w)
        d.set_transforms(*xf(cornell))
        blended = du.apply_morph(cornell.arrays, sets, w)
        st0 = equals_static_upload(cornell, d, blended, "before the errors")
        pd = np.zeros((1, 64, 3), np.float32)

        def refused(call, words):
            with pytest.raises(hjr.HjrError) as e:
                call()
            assert "(%d)" % ERR_ARG in str(e.value) and words in str(e.value), str(e.value)

        refused(lambda: d.set_morph([{"first_vertex": nv - 63, "position_deltas": pd}], [0.0]), "outside the scene")
        refused(lambda: d.set_morph([{"first_vertex": 0, "position_deltas": pd}, {"first_vertex": 63, "position_deltas": pd}], [0.0]), "overlapping")
        refused(lambda: d.set_morph([{"first_vertex": 0, "first_weight": 1, "position_deltas": pd}], [0.0]), "n_weights")
        refused(lambda: d.set_morph_weights(w[:-1]), "weight count")
        refused(lambda: d.update_vertices(nv - 10, np.zeros((11, 3), np.float32)), "outside the scene")
        m = hjr.Morph()
        m.n_sets, m.n_weights = 1, 1
        assert L.hjr_set_morph(d._h, C.byref(m)) == ERR_ARG and b"null sets" in L.hjr_last_error()
        s = (hjr.MorphSet * 1)()
        s[0].first_vertex, s[0].n_vertices, s[0].n_targets = 0, 64, 1
        m.sets = C.addressof(s)
        assert L.hjr_set_morph(d._h, C.byref(m)) == ERR_ARG and b"null position_deltas" in L.hjr_last_error()
        assert L.hjr_update_vertices(d._h, 0, 4, None, None) == ERR_ARG and b"null positions" in L.hjr_last_error()
        assert L.hjr_set_morph_weights(d._h, None, len(w)) == ERR_ARG and b"null weights" in L.hjr_last_error()
        # nothing changed: the same commit is "unchanged", and the next frame is the one before
        d.set_transforms(*xf(cornell))
        st = equals_static_upload(cornell, d, blended, "after the errors")
        assert st["geometry_generation"] == st0["geometry_generation"] and st["morph_vertices"] == 0
        # a non-finite blend is the builders' error; the previous frame data stays current
        bad = w.copy()
        bad[0] = np.float32(np.inf)
        d.set_morph_weights(bad)
        with pytest.raises(hjr.HjrError, match="non-finite vertex"):
            d.set_transforms(*xf(cornell))
        c, _, _ = d.render(cornell.hjr_params(W, H, SPP))
        bits_equal(c, oracle_frame(cornell, blended)[0], "after the non-finite blend")
        d.set_morph_weights(w)
        d.set_transforms(*xf(cornell))
        equals_static_upload(cornell, d, blended, "after good weights again")
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------------------- 6. file level
CLI = os.path.join(hjr.PKG_DIR, "henjou_cli")


def test_cli_morph_targets_key(tmp_path):
    """henjou_cli on a generated glTF with one morphed mesh (three primitives sharing two weights) and a `weights` channel, frames 1..3:
    with "morph_targets": true the PNGs are the oracle's frames of the independently evaluated weights and blend, with device_bvh 0 (the
    overlapped and the serial loop) and 1 (with refits), through the rank path, and with "devices": 2; without the key they are the rest-pose frames."""
    import torch
    assert os.path.exists(CLI), "henjou_cli is not built"
    work = tmp_path / "run"
    gdir = work / "Model" / "test_gltf"
    desc = du.write_morph_gltf(os.path.join(hjr.ASSETS, "Model", "test_gltf"), str(gdir))
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Image"].update(image_width=W, image_height=H, max_spp=SPP, image_name="m")
    ro["Animation"].update(start_frame=1, end_frame=4)
    ro["GLTF_file"]["gltf_filename"] = "cornell_morph.gltf"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")

    def run(name, section, args=()):
        ro["Image"]["image_name"] = name
        ro["Henjou_HIP"] = section
        (work / "render_option.json").write_text(json.dumps(ro))
        q = subprocess.run([CLI, "render_option.json"] + list(args), cwd=work, capture_output=True, text=True, timeout=120, env=env)
        return q, [work / ("%s_%03d.png" % (name, f)) for f in (1, 2, 3)]

    # the expected frames: an independent reading of the file, the numpy blend, the oracle
    ref = du.read_morph_gltf(str(gdir / "cornell_morph.gltf"))
    (track,) = ref["tracks"]
    cwd = os.getcwd()
    os.chdir(work)
    try:
        (work / "render_option.json").write_text(json.dumps(ro))
        opt = hjr.load_render_option("render_option.json")
        sc = hjr.Scene(opt.gltf_path.decode(), opt.gltf_name.decode(), opt)
    finally:
        os.chdir(cwd)
    rest = sc.arrays()
    inst = [i for i, n in enumerate(rest["instance_animation_id"]) if n == desc["node"]][0]
    first, _ = du.instance_vertex_range(rest, inst)
    sets = []
    for p in ref["primitives"]:
        sets.append({"first_vertex": first, "first_weight": 0, "position_deltas": p["position_deltas"], "normal_deltas": p["normal_deltas"]})
        first += p["position_deltas"].shape[1]
    want, want_rest = [], []
    for f in (1, 2, 3):
        t = f32_time(f, opt.fps)
        w = du.eval_weight_track(ref["defaults"][track["mesh"]], track["times"], track["values"], t)
        op = ob.make_params(W, H, SPP, sc.camera(opt, t).as_dict(), frame=f, seed=opt.seed, integrator=opt.integrator, sky=tuple(opt.scene_sky_default),
                            ibl_intensity=opt.IBL_intensity)
        for arrays, out in ((du.apply_morph(sc.arrays(t), sets, w), want), (sc.arrays(t), want_rest)):
            out.append(hjr.float4_to_srgb8(ob.OracleScene(arrays, ob.MATH_PORTABLE).render(op, want_aovs=False)[0])[::-1])
        assert np.mean(np.any(want[-1] != want_rest[-1], axis=-1)) >= 1.0 / 16.0, "frame %d: the morph is not visible enough" % f

    def check(files, expect, what):
        for f in range(3):
            got = hjr.load_png(str(files[f]))
            assert np.array_equal(got, expect[f]), "%s, frame %d: %d pixels differ" % (what, f + 1, int(np.sum(np.any(got != expect[f], axis=-1))))

    q, files = run("rest", {})
    assert q.returncode == 0, q.stdout + q.stderr
    check(files, want_rest, "without the key")
    single = None
    for name, section in (("h", {"morph_targets": True}), ("hs", {"morph_targets": True, "serial_io": True}),
                          ("d", {"morph_targets": True, "device_bvh": True, "device_bvh_refit": 8})):
        q, files = run(name, section)
        assert q.returncode == 0, q.stdout + q.stderr
        check(files, want, str(section))
        single = single or [p.read_bytes() for p in files]
        assert [p.read_bytes() for p in files] == single
    for name, section in (("rd", {"morph_targets": True, "device_bvh": True}),):
        q, files = run(name, section, ["--rank", "0", "--world", "1"])
        assert q.returncode == 0, q.stdout + q.stderr
        assert [p.read_bytes() for p in files] == single, "rank path, " + str(section)
    q, files = run("two", {"morph_targets": True, "device_bvh": True, "devices": 2})
    if torch.cuda.device_count() == 1:
        assert q.returncode == 1 and "stopping the others" in q.stderr and not files[0].exists(), q.stderr[-1500:]
    else:
        assert q.returncode == 0, q.stderr[-1500:]
        assert [p.read_bytes() for p in files] == single
