"""The firefly clamp on the GPU (option "firefly_clamp"; include/henjou_hip.h "Firefly clamp", DESIGN.md §4 rule 9).

The expected colour is numpy float32: the oracle's per-sample values summed into chunk sums as the render kernels sum them, then the
rule (tests/firefly_util.py).  The GPU must give the same bits and the same count of scaled (pixel, chunk) pairs on both kernel families
and under MIS, for every shape at which the kernel takes another path, sharded or not; the other AOVs must not notice the option; sample
passes are refused; the denoise and file paths carry it; and the clamped frame must be closer to the truth than the plain one.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from firefly_util import f32, firefly_rule, frame_of, moved_camera, oracle_color_chunks
from scene_util import ROOT, Cornell, f32_time, hjr
from test_gpu_progressive import SENTINEL, bits, with_range
from test_gpu_variance import render_var

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
ERR_ARG = -1
NEE, MIS = hjr.INTEGRATOR_NEE, hjr.INTEGRATOR_MIS


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def cam35(cornell):
    """The scene's camera moved to x = 3.5: inside the box, no sky pixel, the glass and the small emitter in view."""
    return moved_camera(cornell.camera, 3.5)


@pytest.fixture(scope="module")
def dev(cornell):
    d = cornell.device()
    yield d
    d.close()


def params(cornell, cam, w, h, spp, **kw):
    return hjr.make_params(w, h, spp, cam, sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity, **kw)


def same(got, want, what):
    eq = bits(got) == bits(want)
    assert eq.all(), "%s: %d of %d values differ" % (what, int((~eq).sum()), eq.size)


def render_on_off(dev, p, shape, kappa):
    """The same call with the option off and with kappa: ((AOVs, variance, stats) off, (AOVs, variance, stats) on).  Leaves the option off."""
    res = []
    for k in (0, kappa):
        dev.set_option("firefly_clamp", k)
        rc, out, var = render_var(dev, p, shape)
        assert rc == 0, hjr.lib().hjr_last_error()
        res.append((out, var, dev.stats()))
    dev.set_option("firefly_clamp", 0)
    return res


def check_against_rule(cornell, dev, cam, w, h, spp, kappa, integ=NEE, what=""):
    """Everything the issue asks of one frame: colour = the numpy rule on the oracle's chunk sums, count = numpy's, albedo / normal /
    variance = the option-off call's bits, untouched pixels = the plain frame's bits.  Returns (count, touched mask)."""
    chunk, g = oracle_color_chunks(cornell, w, h, spp, integ, cam)
    rgb, count, touched = firefly_rule(chunk, g, spp, kappa)
    plain_rgb, zero, _ = firefly_rule(chunk, g, spp, 0)
    (off, off_var, off_st), (on, on_var, on_st) = render_on_off(dev, params(cornell, cam, w, h, spp, integrator=integ), (h, w, 4), kappa)
    print("%s %dx%d %d spp kappa %d: %d of %d (pixel, chunk) pairs scaled (%.2f %%), %d of %d pixels touched"
          % (what, w, h, spp, kappa, count, w * h * chunk.shape[0], 100.0 * count / (w * h * chunk.shape[0]), int(touched.sum()), w * h))
    same(off[0], frame_of(plain_rgb), what + ": plain colour vs the oracle's chunk sums")
    assert off_st["firefly_clamped"] == 0
    same(on[0], frame_of(rgb), what + ": clamped colour vs the numpy rule")
    assert on_st["firefly_clamped"] == count, (on_st["firefly_clamped"], count)
    same(on[1], off[1], what + ": albedo")
    same(on[2], off[2], what + ": normal")
    same(on_var, off_var, what + ": variance")
    assert np.array_equal(bits(on[0])[~touched], bits(off[0])[~touched]), what + ": a pixel with no scaled chunk moved"
    if touched.any():
        assert (bits(on[0])[touched] != bits(off[0])[touched]).any()
    return count, touched


@pytest.mark.parametrize("integ, pipeline", [(NEE, 1), (NEE, 2), (MIS, 0)])
def test_main_case(cornell, cam35, integ, pipeline):
    """48 x 32, 256 spp (m = 32), kappa 4, camera at x = 3.5: NEE on the megakernel and on the wavefront kernels, and MIS (which picks
    the wavefront kernels itself)."""
    d = cornell.device({"pipeline": pipeline} if pipeline else None)
    try:
        count, touched = check_against_rule(cornell, d, cam35, 48, 32, 256, 4, integ, "main case, integrator %d, pipeline %d" % (integ, pipeline))
        assert d.stats()["pipeline"] == (pipeline - 1 if pipeline else 1)
        assert count > 0 and touched.any() and (~touched).any()
    finally:
        d.close()


@pytest.mark.parametrize("w, h, spp, kappa", [(20, 12, 32, 4), (20, 12, 100, 4), (16, 8, 1024, 4), (20, 12, 64, 2), (20, 12, 64, 8)])
def test_shapes(cornell, cam35, dev, w, h, spp, kappa):
    """Ragged edge tiles (20 x 12); 32 spp: m = 4, the smallest that acts; 100 spp: m = 12 and a partial chunk of 4; 1024 spp: granule 16,
    m = 64, the largest median; kappa 2 and 8."""
    g = hjr.sample_granule(spp)
    assert (g, spp // g, spp % g) == {32: (8, 4, 0), 100: (8, 12, 4), 1024: (16, 64, 0), 64: (8, 8, 0)}[spp]
    check_against_rule(cornell, dev, cam35, w, h, spp, kappa, NEE, "shape")


@pytest.mark.parametrize("spp", [24, 8])
def test_frames_the_rule_does_not_act_on(cornell, cam35, dev, spp):
    """24 spp (m = 3) and 8 spp (a single chunk, no chunk sums): the option-off frame's bits and a count of 0, at kappa 1, the strictest."""
    (off, off_var, _), (on, on_var, st) = render_on_off(dev, params(cornell, cam35, 20, 12, spp), (12, 20, 4), 1)
    for a, b, name in zip(on + [on_var], off + [off_var], ("colour", "albedo", "normal", "variance")):
        same(a, b, "%d spp %s" % (spp, name))
    assert st["firefly_clamped"] == 0


def test_option_range_and_generic_path(dev):
    assert dev.get_option("firefly_clamp") in (-1, 0)
    for v in (0, 1, 4, 64):
        dev.set_option("firefly_clamp", v)
        assert dev.get_option("firefly_clamp") == v
    for bad in (65, -2, 1000):
        with pytest.raises(hjr.HjrError, match="firefly_clamp"):
            dev.set_option("firefly_clamp", bad)
    dev.set_option("firefly_clamp", 0)


def test_shards_give_the_one_rank_frame(cornell, cam35, dev):
    """44 x 28 (6 x 4 tiles, ragged), 64 spp, kappa 4.  Three ranks on one GPU with HJR_FLAG_PACKED unpack to the one-rank frame and
    their counts add up to its count; HJR_FLAG_ZERO_UNOWNED writes the owned pixels and zeros elsewhere, as for the plain frame."""
    w, h, spp = 44, 28, 64
    dev.set_option("firefly_clamp", 4)
    try:
        rc, full, full_var = render_var(dev, params(cornell, cam35, w, h, spp), (h, w, 4))
        assert rc == 0, hjr.lib().hjr_last_error()
        n_full = dev.stats()["firefly_clamped"]
        assert n_full > 0
        frames = [np.zeros((h, w, 4), f32) for _ in range(3)]
        var = np.zeros((h, w, 4), f32)
        total = 0
        for rank in range(3):
            n = hjr.owned_tiles(w, h, rank, 3)
            rc, out, v = render_var(dev, params(cornell, cam35, w, h, spp, rank=rank, world_size=3, flags=hjr.FLAG_PACKED), (n, 64, 4))
            assert rc == 0, hjr.lib().hjr_last_error()
            total += dev.stats()["firefly_clamped"]
            for f, o in zip(frames, out):
                hjr.unpack_tiles(o, f, rank, 3)
            v4 = np.zeros((n, 64, 4), f32)
            v4[..., 0] = v
            hjr.unpack_tiles(v4, var, rank, 3)
        for f, o, name in zip(frames, full, ("colour", "albedo", "normal")):
            same(f, o, "3 packed ranks, " + name)
        same(var[..., 0], full_var, "3 packed ranks, variance")
        assert total == n_full
        rc, out, v = render_var(dev, params(cornell, cam35, w, h, spp, rank=1, world_size=3, flags=hjr.FLAG_ZERO_UNOWNED), (h, w, 4))
        assert rc == 0, hjr.lib().hjr_last_error()
        own = hjr.owned_tile_mask(w, h, 1, 3)
        same(out[0], np.where(own[..., None], full[0], f32(0)), "ZERO_UNOWNED colour")
        same(v, np.where(own, full_var, f32(0)), "ZERO_UNOWNED variance")
    finally:
        dev.set_option("firefly_clamp", 0)


def test_device_pointers(cornell, cam35, dev):
    """hjr_render_device and hjr_render_device_var into torch tensors on the caller's stream: the host call's bits."""
    import torch
    w, h = 20, 12
    p = params(cornell, cam35, w, h, 64)
    dev.set_option("firefly_clamp", 4)
    try:
        rc, want, want_var = render_var(dev, p, (h, w, 4))
        assert rc == 0 and dev.stats()["firefly_clamped"] > 0
        st = torch.cuda.current_stream().cuda_stream
        for with_var in (False, True):
            color = torch.full((h, w, 4), float(SENTINEL), device="cuda")
            var = torch.full((h, w), float(SENTINEL), device="cuda")
            dev.render_device(p, color.data_ptr(), stream=st, d_variance=var.data_ptr() if with_var else None)
            torch.cuda.synchronize()
            same(color.cpu().numpy(), want[0], "hjr_render_device%s" % ("_var" if with_var else ""))
            if with_var:
                same(var.cpu().numpy(), want_var, "hjr_render_device_var variance")
    finally:
        dev.set_option("firefly_clamp", 0)


def test_sample_passes(cornell, cam35, dev):
    """With the option on the pass [0, g) of a 64 spp frame is HJR_ERR_ARG, names the option and leaves its outputs untouched, through
    hjr_render_var and hjr_render_denoised; the whole range [0, 64) is the one-shot clamped frame; with the option off passes work as before."""
    w, h, spp = 20, 12, 64
    p = params(cornell, cam35, w, h, spp)
    g = hjr.sample_granule(spp)
    rc, plain, plain_var = render_var(dev, p, (h, w, 4))
    assert rc == 0
    dev.set_option("firefly_clamp", 4)
    try:
        rc, one, one_var = render_var(dev, p, (h, w, 4))
        assert rc == 0 and dev.stats()["firefly_clamped"] > 0
        for b, e in ((0, g), (0, 32), (8, 64)):
            rc, out, var = render_var(dev, with_range(p, b, e), (h, w, 4))
            assert rc == ERR_ARG and b"firefly_clamp" in hjr.lib().hjr_last_error(), (b, e, rc)
            assert all((a == SENTINEL).all() for a in out) and (var == SENTINEL).all()
        canary = np.full((h, w, 4), SENTINEL, f32)
        rc = hjr.lib().hjr_render_denoised(dev._h, C.byref(with_range(p, 0, g)), hjr.MODE_DENOISE, canary.ctypes.data, w, h)
        assert rc == ERR_ARG and b"firefly_clamp" in hjr.lib().hjr_last_error() and (canary == SENTINEL).all()
        rc, out, var = render_var(dev, with_range(p, 0, spp), (h, w, 4))
        assert rc == 0, hjr.lib().hjr_last_error()
        for a, b_, name in zip(out + [var], one + [one_var], ("colour", "albedo", "normal", "variance")):
            same(a, b_, "[0, spp) vs one-shot, " + name)
        assert (bits(one[0]) != bits(plain[0])).any()
    finally:
        dev.set_option("firefly_clamp", 0)
    for b, e in ((0, g), (g, 32), (32, spp)):
        rc, out, var = render_var(dev, with_range(p, b, e), (h, w, 4))
        assert rc == 0, hjr.lib().hjr_last_error()
    for a, b_, name in zip(out + [var], plain + [plain_var], ("colour", "albedo", "normal", "variance")):
        same(a, b_, "option off, last pass vs one-shot, " + name)


def test_render_denoised_filters_the_clamped_frame(cornell, cam35, dev):
    """hjr_render_denoised in Denoise mode with the option on = hjr_denoise of the clamped frame's AOVs, and not of the plain frame's;
    with "denoise_variance" the variance-guided filter gets the raw variance."""
    w, h = 44, 28
    p = params(cornell, cam35, w, h, 64)
    plain = dev.render(p)
    dev.set_option("firefly_clamp", 4)
    try:
        c, a, n, v = dev.render(p, want_variance=True)
        assert dev.stats()["firefly_clamped"] > 0
        got = dev.render_denoised(p, hjr.MODE_DENOISE)
        same(got, dev.denoise(hjr.MODE_DENOISE, c, a, n), "Denoise")
        assert not np.array_equal(got, dev.denoise(hjr.MODE_DENOISE, *plain))
        dev.set_option("denoise_variance", 1)
        same(dev.render_denoised(p, hjr.MODE_DENOISE), dev.denoise(hjr.MODE_DENOISE, c, a, n, variance=v), "Denoise, variance-guided")
    finally:
        dev.set_option("denoise_variance", 0)
        dev.set_option("firefly_clamp", 0)


def test_cli_writes_the_clamped_frame(tmp_path):
    """henjou_cli on a 64 x 40 x 64 spp file with "firefly_clamp": 4 writes the PNG of the C-ABI frame with the option on (and not the plain
    one's); the rank path as a world of one writes the same bytes; --devices 2 behaves as tests/test_gpu_cli.py expects: on a box with one
    GPU the launcher stops the job, with more the PNG is the single-GPU run's; the key with "passes" is refused."""
    import torch
    assert os.path.exists(CLI), "henjou_cli is not built"
    work = tmp_path / "run"
    shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Image"].update(image_width=64, image_height=40, max_spp=64, image_name="ff")
    ro["Animation"].update(start_frame=1, end_frame=2)
    ro["Henjou_HIP"] = {"seed": 3, "firefly_clamp": 4}
    (work / "render_option.json").write_text(json.dumps(ro))
    (work / "fps.txt").write_text("24")
    r = subprocess.run([CLI, "render_option.json"], cwd=work, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    single = (work / "ff_001.png").read_bytes()
    cwd = os.getcwd()
    os.chdir(work)
    try:
        opt = hjr.load_render_option("render_option.json")
        sc = hjr.Scene(opt.gltf_path.decode(), opt.gltf_name.decode(), opt)
    finally:
        os.chdir(cwd)
    t = f32_time(1, opt.fps)
    arrays = sc.arrays(t)
    d = hjr.Device(0)
    try:
        d.upload_scene(sc.view)
        d.set_transforms(arrays["transforms"], arrays["inv_transforms"])
        p = hjr.make_params(64, 40, 64, sc.camera(opt, t), frame=1, seed=3, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)
        plain = d.render(p, want_aovs=False)[0]
        d.set_option("firefly_clamp", 4)
        clamped = d.render(p, want_aovs=False)[0]
        assert d.stats()["firefly_clamped"] > 0
    finally:
        d.close()
    got = hjr.load_png(str(work / "ff_001.png"))
    assert np.array_equal(got, hjr.float4_to_srgb8(clamped)[::-1])
    assert not np.array_equal(got, hjr.float4_to_srgb8(plain)[::-1])
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    ro["Image"]["image_name"] = "rank"
    (work / "render_option.json").write_text(json.dumps(ro))
    q = subprocess.run([CLI, "render_option.json", "--rank", "0", "--world", "1"], cwd=work, capture_output=True, text=True, timeout=300, env=env)
    assert q.returncode == 0, q.stdout + q.stderr
    assert (work / "rank_001.png").read_bytes() == single
    ro["Image"]["image_name"] = "two"
    (work / "render_option.json").write_text(json.dumps(ro))
    q = subprocess.run([CLI, "render_option.json", "--devices", "2"], cwd=work, capture_output=True, text=True, timeout=120, env=env)
    if torch.cuda.device_count() == 1:
        assert q.returncode == 1 and "stopping the others" in q.stderr and not (work / "two_001.png").exists(), q.stderr[-1500:]
    else:
        assert q.returncode == 0, q.stderr[-1500:]
        assert (work / "two_001.png").read_bytes() == single
    for extra in ({"passes": 2}, {"noise_threshold": 0.05}):
        ro["Henjou_HIP"] = dict({"seed": 3, "firefly_clamp": 4}, **extra)
        (work / "render_option.json").write_text(json.dumps(ro))
        for args in ([], ["--rank", "0", "--world", "1"]):
            q = subprocess.run([CLI, "render_option.json"] + args, cwd=work, capture_output=True, text=True, timeout=120, env=env)
            assert q.returncode != 0 and "firefly_clamp" in q.stderr and list(extra)[0] in q.stderr, q.stderr[-1500:]


def rmse(a, ref, mask):
    d = (a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64))[mask]
    return float(np.sqrt(np.mean(d * d)))


def test_quality(cornell, cam35, dev):
    """The point of the feature.  48 x 32, NEE, seed 1, 256 spp against an 8192 spp frame of seed 7; pixels of the reference with a
    channel >= 3, or within 1e-3 of the sky's 0.8, are out.  From the camera at x = 3.5 (no sky: mask 100 %) the RMSE of the kappa = 4
    frame must be below half the plain frame's.  Rehearsed on the CPU oracle: 0.0346 against 0.1142 (ratio 0.30); the factor 0.5 is the
    margin for a different reference frame.  The same measure from the scene's own camera is printed, not asserted."""
    res = {}
    for name, cam in (("x = 3.5", cam35), ("the scene's own", cornell.camera)):
        ref = dev.render(params(cornell, cam, 48, 32, 8192, seed=7), want_aovs=False)[0]
        mask = ~((ref[..., :3] >= 3.0).any(-1) | (np.abs(ref[..., :3] - f32(0.8)) < 1e-3).all(-1))
        p = params(cornell, cam, 48, 32, 256)
        plain = dev.render(p, want_aovs=False)[0]
        e = {0: rmse(plain, ref, mask)}
        kept = {}
        for kappa in (2, 4, 8):
            dev.set_option("firefly_clamp", kappa)
            try:
                img = dev.render(p, want_aovs=False)[0]
            finally:
                dev.set_option("firefly_clamp", 0)
            e[kappa] = rmse(img, ref, mask)
            kept[kappa] = float(img[..., :3][mask].astype(np.float64).sum() / plain[..., :3][mask].astype(np.float64).sum())
        print("camera %s: mask %.0f %%, RMSE plain %.5f, kappa 2 / 4 / 8: %.5f / %.5f / %.5f, energy kept %.3f / %.3f / %.3f"
              % (name, 100.0 * mask.mean(), e[0], e[2], e[4], e[8], kept[2], kept[4], kept[8]))
        res[name] = (mask, e)
    mask, e = res["x = 3.5"]
    assert mask.all()
    assert e[4] < 0.5 * e[0], (e[4], e[0])
