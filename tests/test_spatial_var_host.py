"""Host-only parts of the spatial variance estimate (hjr_estimate_variance, option "denoise_variance_spatial"; csrc/hjr_denoise.hip.h,
DESIGN.md §11.3): the native checker the GPU kernel is compared with (tests/native/spatial_var_ref.cpp) against an independent numpy
float64 restatement, its pass-through and unknown rules, the "denoise_variance_spatial" key of the render option, and the condition
function of tools/spatial_var_rehearsal.py on a small oracle frame.  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np

from scene_util import ROOT, Cornell, hjr
from spatial_var_util import UNKNOWN, hostile_variance, lower_median, quality_conditions, spatial_var_ref
from test_device_bvh import _option_json

sys.path.insert(0, os.path.join(ROOT, "tools"))
import spatial_var_rehearsal  # noqa: E402

f32 = np.float32
H, W = 13, 21


def _images(seed):
    """Random colours over smooth guides: neighbouring normals / albedos differ by about one phi, so the nine weights are of order 0.1 .. 1
    (far-apart guides would leave the centre alone in its window, and the estimate would be the rounding error of s2 / s0 - mu^2).
    The one-pass form carries an absolute fp32 error of a few ulp of mu^2, so a relative 1e-4 needs windows whose variance is not below
    about mu^2 / 100: exponentially distributed channels (variance = mean^2 / 3 of the luminance) keep every window well above that, where
    uniform ones (mean^2 / variance = 9, and far more in a window of similar taps) do not."""
    rng = np.random.default_rng(seed)
    img = rng.exponential(0.5, (H, W, 4)).astype(f32)
    alb = (0.5 + rng.normal(0, 0.08, (H, W, 4))).astype(f32)
    nrm = (np.array([0, 0, 1, 0]) + rng.normal(0, 0.2, (H, W, 4))).astype(f32)
    return img, alb, nrm


def numpy_estimate(img, alb, nrm):
    """The rule in float64 with np.exp, written with shifted whole-image copies (np.pad edge mode = clamped indices)."""
    img, alb, nrm = (np.asarray(a, np.float64) for a in (img, alb, nrm))
    lum = img[..., 0] + img[..., 1] + img[..., 2]
    pad = lambda a: np.pad(a, [(1, 1), (1, 1)] + [(0, 0)] * (a.ndim - 2), mode="edge")  # noqa: E731
    pl, pa, pn = pad(lum), pad(alb[..., :3]), pad(nrm[..., :3])
    s0 = np.zeros((H, W)); s1 = np.zeros((H, W)); s2 = np.zeros((H, W))
    for dy in range(3):
        for dx in range(3):
            lt, at, nt = pl[dy:dy + H, dx:dx + W], pa[dy:dy + H, dx:dx + W], pn[dy:dy + H, dx:dx + W]
            wn = np.minimum(np.exp(np.maximum(-((nrm[..., :3] - nt) ** 2).sum(-1) / 0.25, -87.0)), 1.0)
            wa = np.minimum(np.exp(np.maximum(-((alb[..., :3] - at) ** 2).sum(-1) / 0.05, -87.0)), 1.0)
            w = wn * wa
            s0 += w; s1 += w * lt; s2 += w * lt * lt
    mu = s1 / s0
    return np.maximum(s2 / s0 - mu * mu, 0.0)


def test_checker_equals_numpy_float64():
    for seed in (21, 22):
        img, alb, nrm = _images(seed)
        got = spatial_var_ref(img, alb, nrm)
        want = numpy_estimate(img, alb, nrm)
        assert got.shape == (H, W) and got.dtype == f32 and (got >= 0).all() and (got < UNKNOWN).all()
        big = want > 1e-6
        assert big.mean() > 0.95
        assert (np.abs(got[big] - want[big]) <= 1e-4 * want[big]).all(), float(np.max(np.abs(got[big] - want[big]) / want[big]))
        assert (got[~big] <= 2e-6).all()
        assert np.array_equal(spatial_var_ref(img, alb, nrm, np.full((H, W), UNKNOWN, f32)), got), "no input = every pixel unknown"


def test_checker_constant_image_is_exactly_zero():
    """Constant colour and constant guides: every weight is p_exp(-0) = 1, the luminance 1.75 and its square 3.0625 are dyadic, so the
    nine-term sums 9, 15.75 and 27.5625 and both quotients are exact and the difference is +0.  (Under varying guides the weights are
    not dyadic, s1 / s0 rounds, and a constant colour gives a few ulp of mu^2 instead: about 2e-7 here.)"""
    img = np.zeros((H, W, 4), f32)
    img[..., 0], img[..., 1], img[..., 2], img[..., 3] = 0.25, 0.5, 1.0, 1.0
    alb = np.full((H, W, 4), 0.5, f32)
    nrm = np.zeros((H, W, 4), f32)
    nrm[..., 2] = 1
    assert (spatial_var_ref(img, alb, nrm).view(np.uint32) == 0).all()
    _, alb, nrm = _images(23)
    assert spatial_var_ref(img, alb, nrm).max() <= 1e-6


def test_checker_pass_through_and_unknown_rules():
    """0, negative, NaN, -Inf and 0.999e30 are known: kept as stored, to the bit.  +Inf, 1e30 and above are unknown: estimated."""
    img, alb, nrm = _images(24)
    est = spatial_var_ref(img, alb, nrm)
    vin = np.full((H, W), UNKNOWN, f32)
    cases = [(0.0, True), (-0.0, True), (-1.0, True), (np.nan, True), (-np.inf, True), (0.999e30, True), (0.37, True),
             (np.inf, False), (1e30, False), (2e30, False)]
    for k, (v, known) in enumerate(cases):
        vin[k, k + 2] = v
    out = spatial_var_ref(img, alb, nrm, vin)
    for k, (v, known) in enumerate(cases):
        want = vin[k, k + 2] if known else est[k, k + 2]
        assert out[k, k + 2].view(np.uint32) == np.asarray(want, f32).view(np.uint32), "case %r" % v
    untouched = np.ones((H, W), bool)
    for k in range(len(cases)):
        untouched[k, k + 2] = False
    assert np.array_equal(out[untouched], est[untouched]), "a pixel reads its own input only"
    # the checkerboard the GPU test uses: every pixel is one of the two
    vin = hostile_variance(H, W)
    out = spatial_var_ref(img, alb, nrm, vin)
    unknown = ~(np.minimum(np.maximum(np.nan_to_num(vin, nan=0.0, posinf=np.inf, neginf=-np.inf), 0), f32(1e30)) < f32(1e30))
    assert unknown.any() and (~unknown).any() and np.isnan(vin[~unknown]).any() and np.isinf(vin[unknown]).any()
    assert np.array_equal(out[unknown], est[unknown])
    assert np.array_equal(out[~unknown].view(np.uint32), vin[~unknown].view(np.uint32))


def test_render_option_parses_denoise_variance_spatial(tmp_path):
    """"Henjou_HIP": {"denoise_variance_spatial": true} is bit 10 of hjr_render_option.device_bvh_opt: off by default, next to the other
    keys of that field and of denoise_variance, and the struct does not grow for it."""
    load = lambda extra: hjr.load_render_option(_option_json(tmp_path, extra))  # noqa: E731
    for extra in (None, {}, {"seed": 3}, {"denoise_variance_spatial": False}, {"denoise_variance_spatial": 0}, {"denoise_variance": True}):
        assert load(extra).device_bvh_opt == 0
    for extra in ({"denoise_variance_spatial": True}, {"denoise_variance_spatial": 1}):
        o = load(extra)
        assert o.device_bvh_opt == 0x400 and o.denoise_variance == 0, "accepted without the two other keys"
    assert load({"denoise_variance_spatial": True, "denoise_variance": True}).denoise_variance == 1
    o = load({"denoise_variance_spatial": True, "denoise_temporal": True, "firefly_clamp": 8, "device_bvh": True, "device_bvh_opt": 2,
              "device_bvh_instances": True, "device_bvh_graft": True})
    assert o.denoise_variance == 2 and o.device_bvh_opt & 0xff == 2 and o.device_bvh_opt & 0x700 == 0x700 and (o.device_bvh_opt >> 16) & 0x7f == 8
    assert hjr.RenderOption.denoise_variance.offset + 4 == C.sizeof(hjr.RenderOption), "nothing was appended"


def test_lower_median_and_condition_function_on_known_tables():
    assert lower_median([4.0, 1.0, 3.0, 2.0]) == 2.0 and lower_median([5.0]) == 5.0
    row = lambda s, p, u: {"e_spatial": s, "e_plain": p, "e_unknown": u, "e_raw": p}  # noqa: E731
    good = {4: row([0.05, 0.2, 0.04, 0.3], [0.06, 0.1, 0.06, 0.06], [0.12, 0.12, 0.12, 0.12])}  # lower medians 0.05 / 0.06 / 0.12
    assert [h for _, h in quality_conditions(good)] == [True, True]
    bad = {4: row([0.07, 0.2, 0.04, 0.3], [0.06, 0.1, 0.06, 0.06], [0.12, 0.12, 0.12, 0.12])}   # 0.07 against 0.06
    assert [h for _, h in quality_conditions(bad)] == [False, True]
    chain = {"e_plain": [0.1] * 3, "e_off": [0.2, 0.2, 0.2], "e_on": [0.1, 0.2, 0.1]}            # frame 2: equal is not below
    assert [h for _, h in quality_conditions(None, {"static": chain})] == [True, False, True]


def test_rehearsal_condition_function_on_a_small_oracle_frame():
    """tools/spatial_var_rehearsal.py on a 48 x 32 oracle frame (reference 256 spp, single frames only): the table is complete and finite,
    the condition function says of it what an independent evaluation says, and the estimate does change the filter's output.  Whether the
    conditions HOLD is asserted where the design fixes them: at 96 x 64 against 4096 spp (tests/test_gpu_spatial_var.py after the full
    rehearsal); at this size a single firefly decides a frame and 1 and 2 spp fail."""
    table, chains = spatial_var_rehearsal.rehearse(Cornell(), 48, 32, 256, chains=False, spps=(2, 8))
    assert chains == {} and sorted(table) == [2, 8]
    for spp, row in table.items():
        assert all(len(row[k]) == 4 and np.isfinite(row[k]).all() and min(row[k]) > 0 for k in ("e_raw", "e_plain", "e_unknown", "e_spatial"))
        assert row["e_spatial"] != row["e_unknown"]
    conds = quality_conditions(table)
    assert len(conds) == 4
    want = []
    for spp in (2, 8):
        med = {k: float(np.sort(v)[1]) for k, v in table[spp].items()}
        want += [med["e_spatial"] < med["e_plain"], med["e_spatial"] < med["e_unknown"]]
    for text, holds in conds:
        print("%s: %s" % (text, "holds" if holds else "FAILS"))
    assert [h for _, h in conds] == want
