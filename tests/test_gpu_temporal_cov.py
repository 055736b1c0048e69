"""Coverage-aware temporal accumulation on the GPU (hjr_render_gbuffer_cov, hjr_temporal_frame.coverage, option
"denoise_temporal_coverage"; csrc/hjr_temporal.hip.h): the coverage pass and the accumulation kernel bit for bit against
the native checker tests/native/temporal_cov_ref.cpp (a brute force over all triangles, rules 2' and 3' restated), the properties the rules
are for (a static sequence accumulates everywhere; under motion mixed pixels restart and full pixels do not tap them), the stateful paths
against the chain of building blocks, and the quality tables of §11.5.

Shapes: the bundled box at 48 x 32 and 43 x 29 (ragged), 16 spp; the default layout (BVH2), "bvh_width" 4 and one "device_bvh" 1 case."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from scene_util import ROOT, Cornell, f32_time, hjr
from temporal_cov_util import (SNAP, conditions_m, conditions_s, format_table_cov, gbuffer_cov_ref, mixed, quality_sequences_cov, reprojection, rows_from_arrays,
                               rows_from_device, temporal_cov_ref)
from temporal_util import MISS, camera_at, moved_consistent
from test_gpu_denoise_shards import render_shards
from test_gpu_progressive import bits
from test_temporal_host import hostile

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
f32 = np.float32
SIZES = [(48, 32), (43, 29)]
SPP = 16
SIDE = 4  # the coverage side of the accumulation tests and of the quality tables
DENOISE_MODES = [hjr.MODE_DENOISE, hjr.MODE_DENOISE_UPSCALE2X]
FIELDS = ("prim", "inst", "t", "b1", "b2", "pos", "ng", "pad")


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def dev(cornell):
    d = cornell.device()
    yield d
    d.close()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def n_tris(cornell):
    return np.asarray(cornell.arrays["indices"]).size // 3


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    same = bits(got) == bits(want)
    assert same.all(), "%s: %d of %d values differ" % (what, int((~same).sum()), same.size)


def assert_records(got, want, what, fields=FIELDS):
    for name in fields:
        same = got[name].view(np.uint32) == want[name].view(np.uint32)
        assert same.all(), "%s, field %s: %d values differ" % (what, name, int((~same).sum()))


_checked = {}


def checker_records(rows, inst, mat, w, h, cam, side):
    """The checker's coverage pass on the triangle rows in prim order (the brute force does not depend on the order; the key makes every
    builder that produces the same vertex bits share one run)."""
    rows = rows[np.argsort(rows[:, 9].view(np.uint32), kind="stable")]
    key = (hashlib.sha1(rows.tobytes()).hexdigest(), w, h, bytes(cam), side)
    if key not in _checked:
        _checked[key] = gbuffer_cov_ref(rows, inst, mat, w, h, cam, side)
    return _checked[key]


# ------------------------------------------------------------------------------------------------------------------ (a) records
@pytest.mark.parametrize("options,w,h", [(dict(), 48, 32), (dict(), 43, 29), (dict(bvh_width=4), 48, 32), (dict(bvh_width=4), 43, 29), (dict(device_bvh=1), 43, 29)],
                         ids=["bvh2-48x32", "bvh2-43x29", "bvh4-48x32", "bvh4-43x29", "device_bvh-43x29"])
def test_records_equal_the_checker(cornell, options, w, h):
    """hjr_render_gbuffer_cov equals the brute-force checker bit for bit in every field for sides 2, 3 and 4; apart from pad its records
    are hjr_render_gbuffer's bytes, and hjr_render_gbuffer still writes pad = 0.  48 x 32 from the scene's camera moved by a third of a pixel (sky around the box: miss
    records that carry counts), 43 x 29 from x = 3.5 (inside the box)."""
    cam = camera_at(cornell, shift=(0.0, 0.02, 0.02)) if (w, h) == (48, 32) else camera_at(cornell, x=3.5)  # (the shift puts the box's outline inside pixels)
    d = cornell.device(options)
    try:
        rows, inst, mat = rows_from_device(d, cornell.arrays)
        shade = d.copy_frame_data(hjr.FRAME_TRI_SHADE).reshape(-1, 16)
        assert np.array_equal(shade[:len(mat), 15].view(np.uint32), mat), "word 15 of a shading row is the material id"
        p = hjr.make_params(w, h, 1, cam)
        plain = d.gbuffer(p)
        assert (plain["pad"] == 0).all()
        assert_records(plain, checker_records(rows, inst, mat, w, h, cam, 0), "plain G-buffer")
        for side in (2, 3, 4):
            g = d.gbuffer(p, coverage=side)
            assert g.shape == (h, w) and g.dtype == hjr.GBUFFER_DTYPE
            assert_records(g, checker_records(rows, inst, mat, w, h, cam, side), "side %d" % side)
            assert_records(g, plain, "side %d against hjr_render_gbuffer" % side, FIELDS[:-1])
            assert ((g["pad"] >> 8) == side * side).all() and ((g["pad"] & 0xff) <= side * side).all()
            miss = g["prim"] == MISS
            assert mixed(g).sum() >= 20 and (~mixed(g)).sum() >= 20
            if (w, h) == (48, 32):
                assert miss.any() and mixed(g)[miss].any() and (g["pad"][miss] == (side * side) * 0x101).any(), "sky pixels: some cut by the box, some full"
                body = g[miss].copy()
                body["pad"] = 0
                assert not body.tobytes().replace(b"\xff\xff\xff\xff", b"").strip(b"\0"), "every other field of a miss record stays 0"
    finally:
        d.close()


def test_both_passes_share_one_centre_ray(cornell):
    """43 x 29 (partial tiles in both directions), the default layout and "bvh_width" 4, sides 2 and 4: with pad zeroed the coverage pass's
    records are hjr_render_gbuffer's byte for byte, and the plain record's pad is 0 everywhere."""
    w, h = 43, 29
    p = hjr.make_params(w, h, 1, camera_at(cornell, x=3.5))
    for options in (dict(), dict(bvh_width=4)):
        d = cornell.device(options)
        try:
            plain = d.gbuffer(p)
            assert plain.shape == (h, w) and (plain["pad"] == 0).all() and (plain["prim"] != MISS).any()
            for side in (2, 4):
                g = d.gbuffer(p, coverage=side).copy()
                assert ((g["pad"] >> 8) == side * side).all()
                g["pad"] = 0
                assert g.tobytes() == plain.tobytes(), "%s, side %d" % (options, side)
        finally:
            d.close()


def test_entry_point_refusals(cornell, dev):
    L = hjr.lib()
    out = np.zeros((8, 8), hjr.GBUFFER_DTYPE)
    p = cornell.hjr_params(8, 8, 1)
    for side in (0, 1, 5, 16, 0xffffffff):
        assert L.hjr_render_gbuffer_cov(dev._h, C.byref(p), side, out.ctypes.data) == -1 and b"side" in L.hjr_last_error()
        assert L.hjr_render_gbuffer_cov_device(dev._h, C.byref(p), side, out.ctypes.data, None) == -1
    assert not out.tobytes().strip(b"\0"), "nothing was written"
    fresh = hjr.Device(0)
    try:
        assert L.hjr_render_gbuffer_cov(fresh._h, C.byref(p), 2, out.ctypes.data) == -5  # HJR_ERR_STATE: no frame data
    finally:
        fresh.close()
    for kw in (dict(world_size=2), dict(flags=hjr.FLAG_PACKED)):
        assert L.hjr_render_gbuffer_cov(dev._h, C.byref(cornell.hjr_params(8, 8, 1, **kw)), 2, out.ctypes.data) == -1
    assert L.hjr_render_gbuffer_cov(dev._h, C.byref(cornell.hjr_params(0, 8, 1)), 2, out.ctypes.data) == -1
    assert L.hjr_render_gbuffer_cov(dev._h, C.byref(p), 2, None) == -1
    for v in (0, 2, 3, 4, -1):
        dev.set_option("denoise_temporal_coverage", v)
        assert dev.get_option("denoise_temporal_coverage") == v
    for v in (1, 5, -2, 16):
        with pytest.raises(hjr.HjrError):
            dev.set_option("denoise_temporal_coverage", v)
    assert dev.get_option("denoise_temporal_coverage") == -1


# ------------------------------------------------------------------------------------------------------------------ rendered frames
_frames = {}


def rendered(cornell, dev, w, h, k, cam, frame, side=SIDE):
    """One rendered frame (16 spp with its variance, the coverage G-buffer from the GPU) with the instances moved by k steps; cached."""
    key = (w, h, k, bytes(cam), frame, side)
    if key not in _frames:
        m, inv = moved_consistent(cornell.arrays, k)
        dev.set_transforms(m, inv)
        p = hjr.make_params(w, h, SPP, cam, frame=frame, sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)
        c, a, n, v = dev.render(p, want_variance=True)
        _frames[key] = {"camera": cam, "transforms": m, "inv_transforms": inv, "gbuffer": dev.gbuffer(p, coverage=side), "color": c, "variance": v, "coverage": side}
    return {k2: (v2.copy() if isinstance(v2, np.ndarray) else v2) for k2, v2 in _frames[key].items()}


def with_history(fr, seed):
    h, w = fr["gbuffer"].shape
    fr["history"] = np.random.default_rng(seed).integers(1, 41, (h, w)).astype(f32)
    return fr


def accumulate_checked(cornell, dev, prev, cur, what):
    got = dev.temporal_accumulate(prev, cur)
    want = temporal_cov_ref(prev, cur, n_tris(cornell))
    for name, g, w in zip(("colour", "variance", "history"), got, want):
        assert_bits(g, w, "%s, %s" % (what, name))
    return got


# ------------------------------------------------------------------------------------------------------------------ (b) no mixed pixel
def wall_cam(cornell, k):
    """Inside the box, facing one wall that fills the frame, moved a little with k."""
    return camera_at(cornell, x=-0.5, shift=(-0.03 * k, 0.02 * k, 0.025 * k))


def test_a_view_without_mixed_pixels_accumulates_as_without_coverage(cornell, dev):
    w, h = 48, 32
    for k in range(3):  # the condition for using this view, on the CPU first
        g = gbuffer_cov_ref(*rows_from_arrays(cornell.arrays), w, h, wall_cam(cornell, k), SIDE)
        assert not mixed(g).any() and (g["prim"] != MISS).all()
    prev_on = prev_off = None
    for k in range(3):
        cur = rendered(cornell, dev, w, h, 0, wall_cam(cornell, k), 1 + k)
        assert (cur["gbuffer"]["pad"] == SIDE * SIDE * 0x101).all(), "every record has same == total"
        on = accumulate_checked(cornell, dev, prev_on, cur, "wall view, frame %d" % k)
        off = dev.temporal_accumulate(prev_off, dict(cur, coverage=0))
        for a, b in zip(on, off):
            assert_bits(a, b, "coverage on against off, frame %d" % k)
        prev_on = dict(cur, color=on[0], variance=on[1], history=on[2])
        prev_off = dict(cur, coverage=0, color=off[0], variance=off[1], history=off[2])
    assert (on[2] > 2.5).mean() > 0.8, "the sequence does accumulate"


# ------------------------------------------------------------------------------------------------------------------ (c) against the checker
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("case", ["static", "moved", "camera", "no_prev", "hostile", "prev_without_coverage", "cur_without_coverage"])
def test_accumulate_equals_the_checker(cornell, dev, w, h, case):
    cam0 = camera_at(cornell, x=3.5)
    cam1 = camera_at(cornell, x=3.5, turn=0.04, shift=(-0.05, 0.03, 0.06)) if case == "camera" else cam0
    k0, k1 = (1, 2) if case == "moved" else (0, 0)
    prev = with_history(rendered(cornell, dev, w, h, k0, cam0, 1), w * h)
    cur = rendered(cornell, dev, w, h, k1, cam1, 2)
    assert mixed(cur["gbuffer"]).sum() >= 20 and mixed(prev["gbuffer"]).sum() >= 20
    if case == "prev_without_coverage":
        prev["coverage"] = 0
    if case == "cur_without_coverage":
        cur["coverage"] = 0
    if case == "hostile":  # garbage in pad, prim and instance ids out of range, non-finite positions, on both sides
        rng = np.random.default_rng(w)
        hostile(cur, False)
        hostile(prev, True)
        for side in (prev, cur):
            junk = rng.random((h, w)) < 0.3
            side["gbuffer"]["pad"][junk] = rng.integers(0, 2 ** 32, int(junk.sum()), dtype=np.uint64).astype(np.uint32)
        for word, (y, x) in zip((0xffffffff, 0, 5, 0x1410, 0x0900, 0x100f), ((3, 3), (3, 4), (3, 5), (3, 6), (3, 7), (3, 8))):
            prev["gbuffer"]["pad"][y, x] = cur["gbuffer"]["pad"][y, x] = word
    got = accumulate_checked(cornell, dev, None if case == "no_prev" else prev, cur, "%s %dx%d" % (case, w, h))
    if case == "no_prev":
        assert (got[2] == 1).all() and np.array_equal(got[0], cur["color"]) and np.array_equal(got[1], cur["variance"])
    else:
        assert (got[2] > 1).mean() > 0.4, "most pixels find their history (%.0f %%)" % (100 * (got[2] > 1).mean())
    if case == "hostile":
        assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    if case in ("moved", "camera"):
        plain = dev.temporal_accumulate(dict(prev, coverage=0), dict(cur, coverage=0))
        assert not np.array_equal(plain[2], got[2]), "the rules act on this pair"


# ------------------------------------------------------------------------------------------------------------------ (d) static sequence
def test_static_sequence_accumulates_everywhere(cornell, dev):
    """After four static frames every hit pixel has h = 4, mixed or not: a mixed pixel's reprojection lands on its own centre up to
    rounding, inside the snap, and its pad word equals its previous one.  (With rule 3' alone and no rule 2', mixed pixels would tap full
    neighbours only with weights near 0 or restart.)"""
    w, h = 48, 32
    cam = camera_at(cornell, x=3.5)
    prev = None
    for f in range(1, 5):
        cur = rendered(cornell, dev, w, h, 0, cam, f)
        c, v, hist = dev.temporal_accumulate(prev, cur)
        prev = dict(cur, color=c, variance=v, history=hist)
    g = cur["gbuffer"]
    hit = g["prim"] != MISS
    m = mixed(g)
    assert (m & hit).sum() >= 20
    assert np.abs(hist[hit] - 4).max() <= 1e-4, "%d hit pixels (%d of them mixed) are not at h = 4" % (int((np.abs(hist - 4) > 1e-4)[hit].sum()), int((np.abs(hist - 4) > 1e-4)[hit & m].sum()))
    assert (hist[m & hit] == 4).all(), "a mixed pixel's one tap has weight 1: exactly 4"


# ------------------------------------------------------------------------------------------------------------------ (e) sequence M
def test_moving_sequence_restarts_mixed_pixels_and_shields_full_ones(cornell, dev):
    """Every instance moves by frame * (0.05, -0.03, 0.02), camera at x = 3.5 (chosen with the checker on the CPU: at least 20 mixed pixels
    at 48 x 32 in every frame).  Every mixed current pixel outside the snap has h = 1, and no full pixel's result depends on a mixed tap:
    perturbing the previous colour, variance and history at the previous frame's mixed pixels changes no output bit of a full pixel."""
    w, h = 48, 32
    cam = camera_at(cornell, x=3.5)
    prev = None
    outside_total = 0
    for f in range(1, 5):
        arrays = dict(cornell.arrays)
        arrays["transforms"], arrays["inv_transforms"] = moved_consistent(cornell.arrays, f)
        assert mixed(gbuffer_cov_ref(*rows_from_arrays(arrays), w, h, cam, SIDE)).sum() >= 20, "CPU choice of the camera, frame %d" % f
        cur = rendered(cornell, dev, w, h, f, cam, f)
        m_cur = mixed(cur["gbuffer"])
        assert m_cur.sum() >= 20, "frame %d has %d mixed pixels" % (f, int(m_cur.sum()))
        got = accumulate_checked(cornell, dev, prev, cur, "sequence M, frame %d" % f)
        if prev is not None:
            xp, yp = reprojection(prev, cur)
            off = np.maximum(np.abs(xp - np.floor(xp + 0.5)), np.abs(yp - np.floor(yp + 0.5)))
            outside = m_cur & (cur["gbuffer"]["prim"] != MISS) & (off > float(SNAP) + 1e-3)
            outside_total += int(outside.sum())
            assert (got[2][outside] == 1).all(), "frame %d: a mixed pixel outside the snap kept a history" % f
            m_prev = mixed(prev["gbuffer"])
            poisoned = dict(prev, color=prev["color"].copy(), variance=prev["variance"].copy(), history=prev["history"].copy())
            poisoned["color"][m_prev] += f32(100)
            poisoned["variance"][m_prev] += f32(7)
            poisoned["history"][m_prev] = f32(40)
            again = dev.temporal_accumulate(poisoned, cur)
            full = ~m_cur
            for a, b, name in zip(got, again, ("colour", "variance", "history")):
                assert np.array_equal(bits(a)[full], bits(b)[full]), "frame %d: a full pixel's %s depends on a mixed tap" % (f, name)
            without = [dev.temporal_accumulate(dict(q, coverage=0), dict(cur, coverage=0))[0] for q in (prev, poisoned)]
            assert not np.array_equal(bits(without[0])[full], bits(without[1])[full]), "frame %d: without coverage full pixels do tap them" % f
        prev = dict(cur, color=got[0], variance=got[1], history=got[2])
    assert outside_total >= 20


# ------------------------------------------------------------------------------------------------------------------ (f) end to end
W3, H3 = 43, 29


def by_hand(d, p, mode, xf, prev, side=SIDE):
    """render with the variance -> coverage G-buffer -> accumulate against `prev` -> variance-guided filter; (image, the new history)."""
    c, a, n, v = d.render(p, want_variance=True)
    cur = {"camera": hjr.Camera.from_buffer_copy(p.camera), "transforms": xf[0], "inv_transforms": xf[1], "gbuffer": d.gbuffer(p, coverage=side), "color": c, "variance": v,
           "coverage": side}
    tc, tv, th = d.temporal_accumulate(prev, cur)
    return d.denoise(mode, tc, a, n, variance=tv), dict(cur, color=tc, variance=tv, history=th)


def chain(cornell, d, mode, frames=(1, 2, 3), side=SIDE):
    out, prev = [], None
    for f in frames:
        xf = moved_consistent(cornell.arrays, f)
        d.set_transforms(*xf)
        img, prev = by_hand(d, cornell.hjr_params(W3, H3, SPP, frame=f), mode, xf, prev, side)
        out.append(img)
    return out


@pytest.mark.parametrize("mode", DENOISE_MODES, ids=["Denoise", "DenoiseUpScale2X"])
def test_render_denoised_and_shards_equal_the_chain(torch, cornell, mode):
    """hjr_render_denoised with both options equals the chain of building blocks bit for bit over three moving frames, and so does
    hjr_denoise_shards_device on three emulated shards; with the coverage option alone, or at 0, the frames are today's."""
    d, r = cornell.device(), cornell.device()
    try:
        want = chain(cornell, d, mode)
        plain = chain(cornell, d, mode, side=0)
        assert not any(np.array_equal(a, b) for a, b in zip(want[1:], plain[1:])), "the coverage rules change the frames"
        assert_bits(want[0], plain[0], "a first frame has no history: the same image")
        for ctx in (d, r):
            ctx.set_option("denoise_temporal", 1)
            ctx.set_option("denoise_temporal_coverage", SIDE)
        for f, img in zip((1, 2, 3), want):
            xf = moved_consistent(cornell.arrays, f)
            d.set_transforms(*xf)
            r.set_transforms(*xf)
            p = cornell.hjr_params(W3, H3, SPP, frame=f)
            assert_bits(d.render_denoised(p, mode), img, "hjr_render_denoised, frame %d" % f)
            buf, s = render_shards(torch, r, cornell, W3, H3, SPP, 3, True, frame=f)
            ow, oh = (2 * W3, 2 * H3) if mode == hjr.MODE_DENOISE_UPSCALE2X else (W3, H3)
            assert_bits(r.denoise_shards(p, mode, s, ow, oh), img, "hjr_denoise_shards_device, 3 shards, frame %d" % f)
        # setting the option drops the history; at 0 the frames are the plain temporal path's
        d.set_option("denoise_temporal_coverage", 0)
        for f, img in zip((1, 2, 3), plain):
            d.set_transforms(*moved_consistent(cornell.arrays, f))
            assert_bits(d.render_denoised(cornell.hjr_params(W3, H3, SPP, frame=f), mode), img, "coverage 0, frame %d" % f)
        d.set_option("denoise_temporal_coverage", 2)
        d.set_transforms(*moved_consistent(cornell.arrays, 3))
        assert_bits(d.render_denoised(cornell.hjr_params(W3, H3, SPP, frame=3), mode), by_hand(d, cornell.hjr_params(W3, H3, SPP, frame=3), mode,
                                                                                                moved_consistent(cornell.arrays, 3), None)[0], "after setting the option: no history")
        # without "denoise_temporal" the option has no effect
        d.set_option("denoise_temporal", 0)
        d.set_option("denoise_variance", 1)
        p = cornell.hjr_params(W3, H3, SPP, frame=3)
        c, a, n, v = d.render(p, want_variance=True)
        assert_bits(d.render_denoised(p, mode), d.denoise(mode, c, a, n, variance=v), "denoise_temporal off")
    finally:
        d.close()
        r.close()


def test_cli_key_writes_the_png_of_the_chain(cornell, tmp_path):
    """henjou_cli, Render_mode Denoise, frames 1..3 with "denoise_temporal" and "denoise_temporal_coverage": 4: the PNGs are the chain's
    (single process and the rank path as a world of one); --devices 2 behaves as tests/test_gpu_cli.py expects (one GPU: the launcher stops
    the job; more: the single-GPU PNG); the value 1 is refused.  (The bundled file's animation moves nothing within these frames, and on a
    static sequence the rules change an image by rounding only, below 8 bits: that the PNGs differ from a run without the key cannot be
    asserted here; that the context option changes moving frames is asserted on the context, above.)"""
    import torch
    assert os.path.exists(CLI), "henjou_cli is not built"
    work = tmp_path / "run"
    shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Image"].update(image_width=48, image_height=32, max_spp=SPP, image_name="cov")
    ro["Animation"].update(start_frame=1, end_frame=4)
    ro["Render_mode"] = "Denoise"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")

    def run(name, section, args=()):
        ro["Image"]["image_name"] = name
        ro["Henjou_HIP"] = section
        (work / "render_option.json").write_text(json.dumps(ro))
        q = subprocess.run([CLI, "render_option.json"] + list(args), cwd=work, capture_output=True, text=True, timeout=120, env=env)
        return q, [work / ("%s_%03d.png" % (name, f)) for f in (1, 2, 3)]
    section = {"denoise_temporal": True, "denoise_temporal_coverage": SIDE}
    q, files = run("cov", section)
    assert q.returncode == 0, q.stdout + q.stderr
    cwd = os.getcwd()
    os.chdir(work)
    try:
        opt = hjr.load_render_option("render_option.json")
        sc = hjr.Scene(opt.gltf_path.decode(), opt.gltf_name.decode(), opt)
    finally:
        os.chdir(cwd)
    d = hjr.Device(0)
    try:
        d.upload_scene(sc.view)
        prev, want = None, []
        for f in (1, 2, 3):
            t = f32_time(f, opt.fps)
            xf = sc.transforms(t)
            d.set_transforms(*xf)
            p = hjr.make_params(48, 32, SPP, sc.camera(opt, t), frame=f, seed=opt.seed, integrator=opt.integrator, sky=tuple(opt.scene_sky_default),
                                ibl_intensity=opt.IBL_intensity)
            img, prev = by_hand(d, p, hjr.MODE_DENOISE, xf, prev)
            want.append(hjr.float4_to_srgb8(img)[::-1])
    finally:
        d.close()
    for f in range(3):
        assert np.array_equal(hjr.load_png(str(files[f])), want[f]), "frame %d" % (f + 1)
    single = [p.read_bytes() for p in files]
    q, files = run("rank", section, ["--rank", "0", "--world", "1"])
    assert q.returncode == 0, q.stdout + q.stderr
    assert [p.read_bytes() for p in files] == single
    q, files = run("two", section, ["--devices", "2"])
    if torch.cuda.device_count() == 1:
        assert q.returncode == 1 and "stopping the others" in q.stderr and not files[0].exists(), q.stderr[-1500:]
    else:
        assert q.returncode == 0, q.stderr[-1500:]
        assert [p.read_bytes() for p in files] == single
    q, _ = run("bad", {"denoise_temporal": True, "denoise_temporal_coverage": 1})
    assert q.returncode != 0 and "denoise_temporal_coverage" in q.stderr


# ------------------------------------------------------------------------------------------------------------------ (g) quality
def test_quality_tables(cornell):
    """§11.2's set-up (96 x 64, NEE, 16 spp per frame, seed 1, frames 1..8, camera at x = 3.5, references of 4096 spp with seed 7, the same
    mask) with a third column: e_cov, the temporal path with the coverage G-buffer of side 4, next to e_var (per-frame filter) and e_tmp
    (temporal path, option off) from the same renders.
    S (static), asserted: §11.2's four conditions with e_cov in place of e_tmp: e_cov(8) < e_var(8), mean e_cov(4..8) < mean e_var(4..8),
    e_cov(8) < e_cov(2), flicker_cov < flicker_var.
    M (instances moved by frame * (0.05, -0.03, 0.02)): the two claims, mean e_cov(4..8) < mean e_tmp(4..8) and e_cov(3) < e_tmp(3), are
    asserted only if they held in all four CPU rehearsals (48 x 32 and 96 x 64, frame seeds 1 and 2: tools/temporal_rehearsal.py --coverage 4);
    M_ASSERT below records the outcome and DESIGN.md §11.5 the tables.  The whole table is printed; tools/temporal_bench.py records it in
    profiles/temporal_coverage.json."""
    d = cornell.device()
    try:
        tables = quality_sequences_cov(cornell, d, SIDE)
    finally:
        d.close()
    failed = []
    for name, conds, asserted in (("S", conditions_s, (True, True, True, True)), ("M", conditions_m, M_ASSERT)):
        print(format_table_cov(name, tables[name]))
        assert min(tables[name]["mask_share"]) >= 0.8
        for (text, holds), must in zip(conds(tables[name]), asserted):
            print("%s   %s: %s%s" % (name, text, "holds" if holds else "FAILS", "" if must else " (not asserted)"))
            if must and not holds:
                failed.append("%s: %s" % (name, text))
    assert not failed, "; ".join(failed)


# (mean e_cov(4..8) < mean e_tmp(4..8), e_cov(3) < e_tmp(3)): whether each held in all four rehearsals (DESIGN.md §11.5 has the numbers)
# Rehearsals (side 4, SNAP 0.125), mean e_cov(4..8) against mean e_tmp(4..8): 48 x 32 seed 1 0.07957 / 0.07797 (fails), seed 2 0.08399 / 0.08329
# (fails), 96 x 64 seed 1 0.06815 / 0.06939, seed 2 0.06467 / 0.06978: not asserted.  e_cov(3) against e_tmp(3): 0.08548 / 0.11433, 0.08682 / 0.11566,
# 0.07265 / 0.12381, 0.06976 / 0.12126: held in all four, asserted.  The one re-tune (SNAP 0.25) left the 48 x 32 figures as they are: not adopted.
M_ASSERT = (False, True)
