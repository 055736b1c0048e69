"""The variance-guided a-trous filter on the GPU (hjr_denoise_var, option "denoise_variance"; csrc/hjr_denoise.hip.h):
bit for bit the native checker tests/native/denoise_var_ref.cpp, the fused hjr_render_denoised path, the argument checks, the file
level, and the point of the feature: against a converged reference its error falls with the sample count and stays below the plain
filter's, whose error does not fall.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from denoise_var_util import UNKNOWN, denoise_var_ref
from scene_util import ROOT, Cornell, hjr
from test_gpu_progressive import bits, with_range

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
f32 = np.float32


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def dev(cornell):
    d = cornell.device()
    yield d
    d.close()


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    same = bits(got) == bits(want)
    assert same.all(), "%s: %d of %d values differ" % (what, int((~same).sum()), same.size)


@pytest.mark.parametrize("w,h,spp", [(40, 24, 24), (7, 5, 16), (7, 5, 4)])
@pytest.mark.parametrize("mode", [hjr.MODE_DENOISE, hjr.MODE_DENOISE_UPSCALE2X])
def test_filter_equals_native_checker(cornell, dev, w, h, spp, mode):
    """A rendered 40 x 24 frame with its own variance (3 chunks); a 7 x 5 frame, where every tap of step 4 and above is clamped, with a
    known variance (16 spp) and with HJR_VARIANCE_UNKNOWN everywhere (4 spp); both Denoise modes."""
    c, a, n, v = dev.render(cornell.hjr_params(w, h, spp), want_variance=True)
    assert (v == UNKNOWN).all() if spp <= 8 else ((v != UNKNOWN).all() and (v > 0).any())
    got = dev.denoise(mode, c, a, n, variance=v)
    want, _ = denoise_var_ref(mode, c, a, n, v)
    assert_bits(got, want, "hjr_denoise_var %dx%d mode %d" % (w, h, mode))
    assert not np.array_equal(got, dev.denoise(mode, c, a, n)), "the plain filter gives another image"


def test_filter_with_hostile_variances(cornell, dev):
    """NaN, negative, infinite and zero variances next to real ones: the GPU clamps as the checker does."""
    w, h = 40, 24
    c, a, n, v = dev.render(cornell.hjr_params(w, h, 24), want_variance=True)
    v = v.copy()
    v[::3, ::5] = np.nan
    v[1::4, 2::7] = -1.0
    v[5, 5], v[6, 6], v[7, 7] = np.inf, -np.inf, 0.0
    v[10:14, 10:30] = UNKNOWN
    got = dev.denoise(hjr.MODE_DENOISE, c, a, n, variance=v)
    assert np.isfinite(got).all()
    assert_bits(got, denoise_var_ref(1, c, a, n, v)[0], "hostile variances")
    assert np.array_equal(dev.denoise(hjr.MODE_DEFAULT, c, a, n, variance=v), c), "Default copies"


@pytest.mark.parametrize("mode", [hjr.MODE_DENOISE, hjr.MODE_DENOISE_UPSCALE2X])
def test_render_denoised_with_and_without_the_option(cornell, mode):
    """Option "denoise_variance" 1: hjr_render_denoised == hjr_render_var followed by hjr_denoise_var, one-shot and in sample passes (the
    running mean filtered with the variance over n = sample_end).  Option 0 (and the default): today's call, which equals the oracle's
    render + the oracle's plain filter."""
    w, h, spp = 70, 37, 24
    d = cornell.device()
    try:
        p = cornell.hjr_params(w, h, spp)
        osc = ob.OracleScene(cornell.arrays, ob.MATH_PORTABLE)
        oc, oa, on, _ = osc.render(cornell.oracle_params(w, h, spp))
        plain = ob.denoise(mode, oc, oa, on)
        assert d.get_option("denoise_variance") == -1
        assert_bits(d.render_denoised(p, mode), plain, "default")
        d.set_option("denoise_variance", 0)
        assert_bits(d.render_denoised(p, mode), plain, "option 0")
        c, a, n, v = d.render(p, want_variance=True)
        want = d.denoise(mode, c, a, n, variance=v)
        d.set_option("denoise_variance", 1)
        got = d.render_denoised(p, mode)
        assert_bits(got, want, "option 1, one-shot")
        assert not np.array_equal(got, plain)
        assert np.array_equal(d.render_denoised(p, hjr.MODE_DEFAULT), c), "Default mode ignores the option"
        d.set_option("denoise_variance", 0)
        steps = []
        for b, e in [(0, 8), (8, 24)]:
            q = with_range(p, b, e)
            c, a, n, v = d.render(q, want_variance=True)
            steps.append(d.denoise(mode, c, a, n, variance=v))
        d.set_option("denoise_variance", 1)
        for (b, e), s in zip([(0, 8), (8, 24)], steps):
            assert_bits(d.render_denoised(with_range(p, b, e), mode), s, "option 1, pass [%d, %d)" % (b, e))
        assert_bits(steps[-1], want, "the last pass is the one-shot image")
        d.set_option("denoise_variance", -1)
        assert_bits(d.render_denoised(p, mode), plain, "option back at its default")
    finally:
        d.close()


def test_argument_checks(cornell, dev):
    img = np.zeros((8, 8, 4), f32)
    var = np.zeros((8, 8), f32)
    with pytest.raises(RuntimeError):
        dev.denoise(hjr.MODE_DENOISE, img, variance=var)  # guides missing
    with pytest.raises(RuntimeError):
        dev.denoise(7, img, img, img, variance=var)
    L = hjr.lib()
    out = np.zeros((8, 8, 4), f32)
    args = (img.ctypes.data, img.ctypes.data, img.ctypes.data)
    assert L.hjr_denoise_var(dev._h, hjr.MODE_DENOISE, 8, 8, *args, None, out.ctypes.data, 8, 8) == -1  # the variance is required
    assert b"variance" in L.hjr_last_error()
    assert L.hjr_denoise_var(dev._h, hjr.MODE_DEFAULT, 8, 8, *args, None, out.ctypes.data, 8, 8) == 0   # ... but not to copy
    assert L.hjr_denoise_var(dev._h, hjr.MODE_DENOISE, 8, 8, *args, var.ctypes.data, out.ctypes.data, 16, 16) == -1  # size rule of the mode
    assert L.hjr_denoise_var(dev._h, hjr.MODE_DENOISE_UPSCALE2X, 8, 8, *args, var.ctypes.data, out.ctypes.data, 8, 8) == -1
    assert L.hjr_denoise_var(dev._h, hjr.MODE_DENOISE, 0, 8, *args, var.ctypes.data, out.ctypes.data, 0, 8) == -1
    assert L.hjr_denoise_var(None, hjr.MODE_DENOISE, 8, 8, *args, var.ctypes.data, out.ctypes.data, 8, 8) == -1
    with pytest.raises(hjr.HjrError):
        dev.set_option("denoise_variance", 2)
    with pytest.raises(ValueError):
        dev.denoise(hjr.MODE_DENOISE, img, img, img, variance=np.zeros((4, 4), f32))


def test_cli_denoise_variance_key(cornell, dev, tmp_path):
    """henjou_cli, Render_mode Denoise, "Henjou_HIP": {"denoise_variance": true}: the PNG of the Python path (render with the variance,
    variance-guided filter, output stage), and not the PNG written without the key (which is the plain filter's)."""
    pngs = {}
    for key in (True, False):
        work = tmp_path / ("run%d" % key)
        shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
        ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
        ro["Image"].update(image_width=96, image_height=64, max_spp=24, image_name="dv")
        ro["Animation"].update(start_frame=1, end_frame=2)
        ro["Render_mode"] = "Denoise"
        if key:
            ro["Henjou_HIP"] = {"denoise_variance": True}
        (work / "render_option.json").write_text(json.dumps(ro))
        p = subprocess.run([CLI, "render_option.json"], cwd=work, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        pngs[key] = hjr.load_png(str(work / "dv_001.png"))
    c, a, n, v = dev.render(cornell.hjr_params(96, 64, 24, frame=1, seed=cornell.opt.seed), want_variance=True)
    exp = hjr.float4_to_srgb8(dev.denoise(hjr.MODE_DENOISE, c, a, n, variance=v))[::-1]
    assert np.array_equal(pngs[True], exp), "%d pixels differ" % int(np.sum(np.any(pngs[True] != exp, axis=-1)))
    plain = hjr.float4_to_srgb8(dev.denoise(hjr.MODE_DENOISE, c, a, n))[::-1]
    assert np.array_equal(pngs[False], plain)
    assert not np.array_equal(pngs[True], pngs[False])


def test_quality_error_falls_with_the_sample_count(cornell, dev):
    """The point of the feature.  Bundled Cornell box, 96 x 64, NEE; reference: 16384 spp with another seed; RMSE over the pixels DESIGN.md
    §11 counts.  The mask comes from the reference's own colour AOV: light sources out (a channel >= 3) and the constant background out
    (all channels within 1e-3 of the sky's 0.8), and must keep at least 80 % of the frame.  From the scene's own camera position 48 % of a
    3:2 frame is background, so the camera is moved forward along its axis from x = 5.39 to x = 3.5, where the box opening (half width 1,
    at x = 1) fills the frame (the frame's half width at distance 2.5 is 1.5 / camera_f * 2.5 = 0.98); nothing else about it changes.
    Required: e_var < e_plain at 64, 256 and 1024 spp (the yardstick is the parent's filter on the same frames), and e_var strictly
    decreasing over 16, 64, 256, 1024 spp.  e_var / e_raw is printed, not asserted (tools/denoise_var_bench.py records it)."""
    w, h = 96, 64
    cam = hjr.Camera.from_buffer_copy(cornell.camera)
    cam.pos[0] = 3.5
    kw = dict(sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)
    ref = dev.render(hjr.make_params(w, h, 16384, cam, seed=7, **kw), want_aovs=False)[0]
    mask = (ref[..., :3].max(axis=-1) < 3.0) & (np.abs(ref[..., :3] - 0.8).max(axis=-1) > 1e-3)
    assert mask.mean() >= 0.8, "the mask keeps %.1f %% of the pixels" % (100 * mask.mean())

    def rmse(img):
        return float(np.sqrt(np.mean((img[..., :3][mask].astype(np.float64) - ref[..., :3][mask]) ** 2)))

    e = {}
    for spp in (16, 64, 256, 1024):
        c, a, n, v = dev.render(hjr.make_params(w, h, spp, cam, seed=1, **kw), want_variance=True)
        e[spp] = (rmse(c), rmse(dev.denoise(hjr.MODE_DENOISE, c, a, n)), rmse(dev.denoise(hjr.MODE_DENOISE, c, a, n, variance=v)))
        print("spp %5d  e_raw %.5f  e_plain %.5f  e_var %.5f  e_var/e_raw %.3f" % ((spp,) + e[spp] + (e[spp][2] / e[spp][0],)))
    for spp in (64, 256, 1024):
        assert e[spp][2] < e[spp][1], "at %d spp: e_var %.5f, e_plain %.5f" % (spp, e[spp][2], e[spp][1])
    ev = [e[spp][2] for spp in (16, 64, 256, 1024)]
    assert ev[0] > ev[1] > ev[2] > ev[3], "e_var is not strictly decreasing: %s" % ev
