"""Temporal luminance moments on the GPU (hjr_temporal_accumulate_moments[_device], option "denoise_temporal_moments";
csrc/hjr_temporal.hip.h section TEMPORAL MOMENTS).  Every comparison of the kernel is GPU == the native checker
tests/native/temporal_moments_ref.cpp, bit for bit on all four outputs (colour, variance, history, moments); then the ABI rules, the context
option against the stateless pieces chained by hand, shards and the file key, and the quality comparison the option is for.

Shapes: the kernel's block is 64 x 4 lanes, so 70 x 9 has partial blocks on both axes; the rendered chains run at 40 x 24 and 48 x 32,
4 spp (a single chunk: the rendered variance is unknown, the 3 x 3 estimate fills it)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from denoise_var_util import denoise_var_ref
from scene_util import ROOT, Cornell, f32_time, hjr
from spatial_var_util import spatial_var_ref
from temporal_cov_util import mixed, reprojection
from temporal_moments_util import MOMENTS_MIN, UNKNOWN, format_tables, quality_chain, quality_conditions, temporal_moments_ref
from temporal_util import MISS, assert_same, camera_at, identity_xf, luminance, moved_consistent, next_prev, plane_gbuffer, same_bits, wall_camera
from test_gpu_denoise_shards import render_shards
from test_gpu_progressive import with_range
from test_temporal_moments_host import hostile_moments

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
f32 = np.float32
ERR_ARG = -1
OPTIONS = ("denoise_temporal", "denoise_variance_spatial", "denoise_temporal_moments")


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


def sky(cornell):
    return dict(sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)


def checked(cornell, dev, prev, cur, what):
    """Device.temporal_accumulate(moments=True) == the checker on all four outputs; returns them."""
    got = dev.temporal_accumulate(prev, cur, moments=True)
    assert len(got) == 4 and got[3].shape == got[1].shape + (2,)
    assert_same(got, temporal_moments_ref(prev, cur, n_tris(cornell)), what)
    return got


def rendered(cornell, dev, w, h, spp, cam, frame, k=0, coverage=0):
    """A rendered frame as the temporal stage sees it: colour, the variance behind the 3 x 3 estimate, the G-buffer; instances moved by k steps."""
    xf = moved_consistent(cornell.arrays, k)
    dev.set_transforms(*xf)
    p = hjr.make_params(w, h, spp, cam, frame=frame, seed=1, **sky(cornell))
    c, a, n, v = dev.render(p, want_variance=True)
    cur = {"camera": cam, "transforms": xf[0], "inv_transforms": xf[1], "gbuffer": dev.gbuffer(p, coverage=coverage), "color": c,
           "variance": dev.estimate_variance(c, a, n, v)}
    if coverage:
        cur["coverage"] = coverage
    return cur


# ------------------------------------------------------------------------------------------------------------------ 1. no previous frame
def test_no_previous_frame(cornell, dev):
    """70 x 9, partial blocks on both axes: m = (l, l * l) everywhere; colour, variance and history are the plain call's."""
    cur = rendered(cornell, dev, 70, 9, 4, camera_at(cornell), 1)
    assert (cur["gbuffer"]["prim"] == MISS).any() and (cur["gbuffer"]["prim"] != MISS).any()
    got = checked(cornell, dev, None, cur, "no previous frame")
    assert_same(got[:3], dev.temporal_accumulate(None, cur), "against the plain call")
    l = luminance(cur["color"])
    assert same_bits(got[3][..., 0], l) and same_bits(got[3][..., 1], l * l) and (got[2] == 1).all()


# ------------------------------------------------------------------------------------------------------------------ 2. static chain
def test_static_chain_crosses_the_switch(cornell, dev):
    """Six static frames, 40 x 24, 4 spp, NEE: compared after every frame.  No pixel has h >= 4 at frame 3 and every hit pixel has at frame 4,
    so the propagated variance (frames 2, 3) and the moments' variance (frames 4..6) are both compared."""
    cam = camera_at(cornell, x=3.5)  # (a static reprojection returns every integer history exactly from here: checked on the CPU)
    prev = None
    for f in range(1, 7):
        cur = rendered(cornell, dev, 40, 24, 4, cam, f)
        got = checked(cornell, dev, prev, cur, "static chain, frame %d" % f)
        hit = cur["gbuffer"]["prim"] != MISS
        assert hit.sum() >= 100 and (~hit).sum() >= 50
        plain = dev.temporal_accumulate(prev, cur)
        assert_same((got[0], got[2]), (plain[0], plain[2]), "colour and history of the plain call, frame %d" % f)
        if f <= 3:
            assert not (got[2] >= MOMENTS_MIN).any(), "frame %d: below the switch everywhere" % f
            assert same_bits(got[1], plain[1]), "frame %d: the propagated variance" % f
        else:
            assert (got[2][hit] >= MOMENTS_MIN).all(), "frame %d: every hit pixel is past the switch" % f
            assert not np.array_equal(got[1][hit], plain[1][hit]) and (got[1][hit] < UNKNOWN).all()
            assert same_bits(got[1][~hit], plain[1][~hit])
        prev = next_prev(cur, got)


# ------------------------------------------------------------------------------------------------------------------ 3. motion
def test_moving_chain_with_a_turning_camera(cornell, dev):
    """Five frames, every instance moved by frame * (0.05, -0.03, 0.02) and the camera turned and shifted a little more each frame: bilinear
    mixing of unlike histories.  At least one pixel ends with a non-integer h in (3, 5) (the switch compares a fractional h), and at least
    one tap is rejected: a hit pixel whose reprojection lies well inside the previous frame restarts only if all four taps were refused."""
    w, h = 40, 24
    prev, fractional, refused = None, 0, 0
    for f in range(1, 6):
        cam = camera_at(cornell, x=3.5, turn=0.03 * f, shift=(-0.072 * f, 0.048 * f, 0.09 * f))  # (chosen with the checker on the CPU: 23 such pixels, 4 refusals)
        cur = rendered(cornell, dev, w, h, 4, cam, f, k=f)
        got = checked(cornell, dev, prev, cur, "moving chain, frame %d" % f)
        if prev is not None:
            xp, yp = reprojection(prev, cur)
            inside = (xp >= 1) & (xp <= w - 2) & (yp >= 1) & (yp <= h - 2)
            refused += int((inside & (got[2] == 1)).sum())
        hh = got[2]
        fractional += int(((hh > 3) & (hh < 5) & (np.abs(hh - np.round(hh)) > 1e-3)).sum())
        prev = next_prev(cur, got)
    assert fractional >= 1 and refused >= 1, (fractional, refused)
    assert (got[2] >= MOMENTS_MIN).any() and (got[2] < MOMENTS_MIN).any()


# ------------------------------------------------------------------------------------------------------------------ 4. hostile input
W4, H4 = 70, 9
WALL = (-4.0, 0, 7, -1e9, 1e9)


def hostile_records(d, prev_side):
    """tests/test_temporal_host.py's kinds of hostile records, placed inside 70 x 9 on rows 0 and 8."""
    g = d["gbuffer"]
    g["prim"][0, 22] = 0xfffffffe; g["prim"][0, 24] = 1 << 30; g["inst"][0, 26] = 2; g["inst"][0, 28] = 0xffffffff; g["inst"][0, 30] = 0x80000000
    g["pos"][8, 22] = np.nan; g["pos"][8, 24] = [np.inf, 0, -4]; g["pos"][8, 26] = [0, -np.inf, np.nan]; g["pos"][8, 28] = [3e38, 3e38, -3e38]
    g["ng"][8, 40] = np.nan; g["ng"][8, 42] = np.inf; g["ng"][8, 44] = 0
    g["pos"][8, 50] = [0, 0, 4]; g["pos"][8, 52] = [0, 0, 0]
    if prev_side:
        d["history"][0, 50] = np.nan; d["history"][0, 52] = -np.inf; d["history"][0, 54] = np.inf


def plane_frame(cam, seed, hist=None, moments=False):
    rng = np.random.default_rng(seed)
    d = {"camera": cam, "transforms": identity_xf(2), "inv_transforms": identity_xf(2), "gbuffer": plane_gbuffer(W4, H4, cam, [WALL, (-2.0, 1, 3, -0.5, 0.5)]),
         "color": rng.uniform(0, 0.25, (H4, W4, 4)).astype(f32), "variance": rng.uniform(0.01, 0.02, (H4, W4)).astype(f32)}
    if hist is not None:
        d["history"] = np.broadcast_to(np.asarray(hist, f32), (H4, W4)).copy()
    if moments:
        d["moments"] = rng.uniform(0.1, 0.9, (H4, W4, 2)).astype(f32)
    return d


@pytest.mark.parametrize("hist", [2.0, 4.0, 30.0])
def test_hostile_moments(cornell, dev, hist):
    """Synthetic plane G-buffers at 70 x 9: NaN, +-Inf, 1e38 (m1 * m1 overflows), 3e38 and a negative m2 in the previous moments, next to
    hostile records and variances on both sides.  Below and above the switch the kernel equals the checker; every variance is "unknown" or
    finite and not negative; colour and history are the plain call's (the moments reach neither)."""
    cam = wall_camera()
    prev, cur = plane_frame(cam, 1, hist=hist, moments=True), plane_frame(cam, 2)
    hostile_moments(prev["moments"])
    prev["moments"][6, 40:64] = np.repeat(np.array([np.nan, np.inf, -np.inf, 1e38, -1e38, 3e38, -4.0, 0.0], f32), 3).reshape(24, 1) * np.ones(2, f32)
    hostile_records(prev, True)
    hostile_records(cur, False)
    prev["variance"][1, 1], prev["variance"][2, 2], prev["variance"][3, 3], cur["variance"][5, 5] = UNKNOWN, np.nan, -1.0, np.inf
    got = checked(cornell, dev, prev, cur, "hostile, h_prev = %g" % hist)
    v = got[1]
    ok = (v == UNKNOWN) | (np.isfinite(v) & (v >= 0) & (v < UNKNOWN))
    plain = dev.temporal_accumulate(prev, cur)
    assert_same((got[0], got[2]), (plain[0], plain[2]), "colour and history")
    restart = got[2] == 1
    assert ok[~restart].all(), "a variance that is neither unknown nor finite"
    assert restart.any() and same_bits(v[restart], cur["variance"][restart])
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    if hist >= 4:
        assert (v == UNKNOWN).sum() >= 20 and (v[6, 58:61] == 0).all()


def test_reprojection_left_of_and_above_the_image(cornell, dev):
    """The camera moves by half a pixel footprint in x and in y, so pixel (0, 0) reprojects to (-0.5, -0.5): xp and yp in [-1, 0), x0 = y0 =
    -1, three taps outside the image and one inside.  Row 0 and column 0 keep a history from the taps that exist."""
    step = (2.0 / H4) * 4.0 / 2.0 * 0.5  # half a footprint on the wall at distance 4 with f = 2
    prev, cur = plane_frame(wall_camera(0.0, 0.0), 3, hist=5.0, moments=True), plane_frame(wall_camera(-step, -step), 4)
    prev["gbuffer"] = plane_gbuffer(W4, H4, prev["camera"], [WALL])
    cur["gbuffer"] = plane_gbuffer(W4, H4, cur["camera"], [WALL])
    xp, yp = reprojection(prev, cur)
    assert -1 <= xp[0, 0] < 0 and -1 <= yp[0, 0] < 0 and (xp[:, 0] < 0).all() and (yp[0, :] < 0).all()
    got = checked(cornell, dev, prev, cur, "reprojection in [-1, 0)")
    assert np.abs(got[2] - 6).max() <= 1e-4, "the one tap inside carries the history"
    # and one more step: everything on row 0 / column 0 falls outside [-1, ...)
    far = plane_frame(wall_camera(-3 * step, -3 * step), 4)
    far["gbuffer"] = plane_gbuffer(W4, H4, far["camera"], [WALL])
    got = checked(cornell, dev, prev, far, "reprojection below -1")
    assert (got[2][0] == 1).all() and (got[2][:, 0] == 1).all() and (got[2][1:, 1:] > 1).all()


# ------------------------------------------------------------------------------------------------------------------ 5. with coverage
def test_coverage_rules_carry_the_moments(cornell, dev):
    """hjr_temporal_kernel<true, true> on the moving coverage sequence of tests/temporal_cov_util.py (every instance moved by frame * (0.05,
    -0.03, 0.02), camera at x = 3.5), 48 x 32, side 2, five frames: mixed pixels snap or restart, full ones refuse mixed taps, and the
    moments ride on the taps that are left."""
    cam = camera_at(cornell, x=3.5)
    prev = None
    for f in range(1, 6):
        cur = rendered(cornell, dev, 48, 32, 4, cam, f, k=f, coverage=2)
        assert mixed(cur["gbuffer"]).sum() >= 20
        got = checked(cornell, dev, prev, cur, "coverage, frame %d" % f)
        if prev is not None:
            off = dev.temporal_accumulate(dict(prev, coverage=0), dict(cur, coverage=0), moments=True)
            assert not np.array_equal(off[3], got[3]), "frame %d: the rules act on the moments" % f
        prev = next_prev(cur, got)
    assert (got[2] >= MOMENTS_MIN).any()


# ------------------------------------------------------------------------------------------------------------------ 6. ABI
def raw_call(dev, prev, cur, prev_moments, out_moments, frame_size=None, fill=7.0):
    """hjr_temporal_accumulate_moments on sentinel-filled outputs: (status, colour, variance, history, moments or None).  frame_size: the
    struct_size both frames claim."""
    keep = []
    fc = hjr.Device._temporal_frame(cur, keep)
    fp = None if prev is None else hjr.Device._temporal_frame(prev, keep)
    for f in (fc, fp):
        if f is not None and frame_size is not None:
            f.struct_size = frame_size
    h, w = fc.height, fc.width
    outs = [np.full((h, w, 4), fill, f32), np.full((h, w), fill, f32), np.full((h, w), fill, f32), np.full((h, w, 2), fill, f32) if out_moments else None]
    pm = None if prev_moments is None else np.ascontiguousarray(prev_moments, f32)
    rc = hjr.lib().hjr_temporal_accumulate_moments(dev._h, None if fp is None else C.byref(fp), C.byref(fc), outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data,
                                                   None if pm is None else pm.ctypes.data, outs[3].ctypes.data if out_moments else None)
    return (rc,) + tuple(outs)


def test_abi_rules(torch, cornell, dev):
    """out_moments == NULL is hjr_temporal_accumulate bit for bit, whatever prev_moments is; out_moments with a previous frame and no
    prev_moments is HJR_ERR_ARG and writes nothing; without a previous frame prev_moments is not needed; hjr_temporal_frame is the
    128-byte struct of callers built before the moments existed (and a 124-byte one, which ends before `coverage`, still works); the device
    form gives the host form's bits."""
    cam = camera_at(cornell, x=3.5)
    first = rendered(cornell, dev, 40, 24, 4, cam, 1)
    o = dev.temporal_accumulate(None, first, moments=True)
    prev, cur = next_prev(first, o), rendered(cornell, dev, 40, 24, 4, cam, 2)
    plain = dev.temporal_accumulate(prev, cur)
    want = dev.temporal_accumulate(prev, cur, moments=True)
    assert C.sizeof(hjr.TemporalFrame) == 128
    for pm in (prev["moments"], None, np.full((24, 40, 2), np.nan, f32)):
        rc, c, v, h, _ = raw_call(dev, prev, cur, pm, False)
        assert rc == 0
        assert_same((c, v, h), plain, "out_moments == NULL")
    rc, c, v, h, m = raw_call(dev, prev, cur, None, True)
    assert rc == ERR_ARG and b"moments" in hjr.lib().hjr_last_error()
    assert all((a == 7).all() for a in (c, v, h, m)), "nothing was enqueued"
    with pytest.raises(hjr.HjrError):
        dev.temporal_accumulate(dict(prev, moments=None), cur, moments=True)
    rc, *got = raw_call(dev, None, cur, None, True)  # no previous frame: nothing to miss
    assert rc == 0 and (got[2] == 1).all()
    for size in (128, 124):
        rc, *got = raw_call(dev, prev, cur, prev["moments"], True, size)
        assert rc == 0
        assert_same(got, want, "%d-byte frames" % size)
    keep = []
    fc, fp = hjr.Device._temporal_frame(cur, keep), hjr.Device._temporal_frame(prev, keep)
    outs = [np.zeros((24, 40, 4), f32), np.zeros((24, 40), f32), np.zeros((24, 40), f32), np.zeros((24, 40, 2), f32)]
    assert hjr.lib().hjr_temporal_accumulate_moments(dev._h, C.byref(fp), C.byref(fc), outs[0].ctypes.data, outs[1].ctypes.data, None, prev["moments"].ctypes.data,
                                                     outs[3].ctypes.data) == ERR_ARG
    # the device form
    t = {}
    for name, d in (("p", prev), ("c", cur)):
        for key in ("transforms", "inv_transforms", "color", "variance", "history", "moments"):
            if d.get(key) is not None:
                t[name + key] = torch.from_numpy(np.ascontiguousarray(d[key], f32)).cuda()
        t[name + "gbuffer"] = torch.from_numpy(np.ascontiguousarray(d["gbuffer"]).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()

    def device_frame(name, d):
        f = hjr.Device._temporal_frame(d, keep)
        f.transforms12, f.inv_transforms12, f.gbuffer = t[name + "transforms"].data_ptr(), t[name + "inv_transforms"].data_ptr(), t[name + "gbuffer"].data_ptr()
        f.color, f.variance = t[name + "color"].data_ptr(), t[name + "variance"].data_ptr()
        f.history = t[name + "history"].data_ptr() if name == "p" else None
        return f
    dp, dc = device_frame("p", prev), device_frame("c", cur)
    d_out = [torch.zeros(s, dtype=torch.float32, device="cuda") for s in ((24, 40, 4), (24, 40), (24, 40), (24, 40, 2))]
    torch.cuda.synchronize()
    L = hjr.lib()
    ptr = lambda a: C.c_void_p(a.data_ptr())
    assert L.hjr_temporal_accumulate_moments_device(dev._h, C.byref(dp), C.byref(dc), ptr(d_out[0]), ptr(d_out[1]), ptr(d_out[2]), ptr(t["pmoments"]), ptr(d_out[3]), None) == 0
    dev.synchronize()
    assert_same([a.cpu().numpy() for a in d_out], want, "device form")
    for a in d_out:
        a.fill_(7)
    torch.cuda.synchronize()
    assert L.hjr_temporal_accumulate_moments_device(dev._h, C.byref(dp), C.byref(dc), ptr(d_out[0]), ptr(d_out[1]), ptr(d_out[2]), None, None, None) == 0
    dev.synchronize()
    assert_same([a.cpu().numpy() for a in d_out[:3]], plain, "device form, out_moments == NULL")
    assert (d_out[3].cpu().numpy() == 7).all()
    assert L.hjr_temporal_accumulate_moments_device(dev._h, C.byref(dp), C.byref(dc), ptr(d_out[0]), ptr(d_out[1]), ptr(d_out[2]), None, ptr(d_out[3]), None) == ERR_ARG
    dev.synchronize()
    assert (d_out[3].cpu().numpy() == 7).all(), "nothing was enqueued"


# ------------------------------------------------------------------------------------------------------------------ 7. the context option
W7, H7, SPP7, FRAMES7 = 48, 32, 4, 8


def by_hand(d, p, mode, xf, prev, moments=True):
    """render with the variance -> 3 x 3 estimate -> G-buffer -> accumulate against `prev` -> variance-guided filter: (image, new history)."""
    c, a, n, v = d.render(p, want_variance=True)
    cur = {"camera": hjr.Camera.from_buffer_copy(p.camera), "transforms": xf[0], "inv_transforms": xf[1], "gbuffer": d.gbuffer(p), "color": c,
           "variance": d.estimate_variance(c, a, n, v)}
    out = d.temporal_accumulate(prev, cur, moments=moments)
    nxt = dict(cur, color=out[0], variance=out[1], history=out[2])
    if moments:
        nxt["moments"] = out[3]
    return d.denoise(mode, out[0], a, n, variance=out[1]), nxt


def frame7(cornell, f, spp=SPP7):
    return cornell.hjr_params(W7, H7, spp, frame=f)


def moved7(cornell, f):
    return moved_consistent(cornell.arrays, min(f, 3))  # the instances move for three frames, then rest: histories of every length up to 8


def hand_chain(cornell, d, mode, moments, frames=range(1, FRAMES7 + 1), spp=SPP7):
    out, prev = [], None
    for f in frames:
        xf = moved7(cornell, f)
        d.set_transforms(*xf)
        img, prev = by_hand(d, frame7(cornell, f, spp), mode, xf, prev, moments)
        out.append(img)
    return out, prev


def set_all(d, value=1):
    for key in OPTIONS:
        d.set_option(key, value)


def test_context_chain_equals_the_pieces(cornell):
    """Eight frames of hjr_render_denoised, 48 x 32, 4 spp, with "denoise_temporal", "denoise_variance_spatial" and the new option: the
    stateless pieces chained by hand, bit for bit, and not the chain without moments once histories reach 4; setting the option drops the
    history; with the option at 0 the frames are the parent's."""
    mode = hjr.MODE_DENOISE
    d = cornell.device()
    try:
        want, last = hand_chain(cornell, d, mode, True)
        without, _ = hand_chain(cornell, d, mode, False)
        assert (last["history"] >= MOMENTS_MIN).mean() > 0.5
        for f in range(FRAMES7):
            assert same_bits(want[f], without[f]) == (f < 3), "frame %d: the moments matter from the fourth frame on" % (f + 1)
        assert d.get_option("denoise_temporal_moments") == -1
        set_all(d)
        assert d.get_option("denoise_temporal_moments") == 1
        for f in range(1, FRAMES7 + 1):
            d.set_transforms(*moved7(cornell, f))
            assert same_bits(d.render_denoised(frame7(cornell, f), mode), want[f - 1]), "frame %d" % f
        # setting the option (to the value it has) drops the history: frame 8 again is a first frame
        d.set_option("denoise_temporal_moments", 1)
        first = by_hand(d, frame7(cornell, FRAMES7), mode, moved7(cornell, FRAMES7), None)[0]
        assert same_bits(d.render_denoised(frame7(cornell, FRAMES7), mode), first) and not same_bits(first, want[-1])
        # option 0: the parent's frames
        d.set_option("denoise_temporal_moments", 0)
        for f in range(1, FRAMES7 + 1):
            d.set_transforms(*moved7(cornell, f))
            assert same_bits(d.render_denoised(frame7(cornell, f), mode), without[f - 1]), "option 0, frame %d" % f
        with pytest.raises(hjr.HjrError):
            d.set_option("denoise_temporal_moments", 2)
        # without "denoise_temporal" it has no effect, and Default mode ignores it
        d.set_option("denoise_temporal_moments", 1)
        d.set_option("denoise_temporal", 0)
        d.set_option("denoise_variance", 1)
        p = frame7(cornell, 3)
        c, a, n, v = d.render(p, want_variance=True)
        assert same_bits(d.render_denoised(p, mode), d.denoise(mode, c, a, n, variance=d.estimate_variance(c, a, n, v)))
        d.set_option("denoise_temporal", 1)
        assert same_bits(d.render_denoised(p, hjr.MODE_DEFAULT), d.render(p, want_aovs=False)[0])
    finally:
        d.close()


def test_two_sample_passes_advance_the_history_once(cornell):
    """Frames of 24 spp rendered in passes of 8 and 16 samples: the first pass computes moments and discards them, the last pass ends on the
    one-shot bits, over six frames (so the moments of frames 4..6 come from histories that advanced once per frame)."""
    mode, spp = hjr.MODE_DENOISE_UPSCALE2X, 24
    d = cornell.device()
    try:
        want, _ = hand_chain(cornell, d, mode, True, frames=range(1, 7), spp=spp)
        without, _ = hand_chain(cornell, d, mode, False, frames=range(1, 7), spp=spp)
        assert not same_bits(want[5], without[5])
        set_all(d)
        for f in range(1, 7):
            d.set_transforms(*moved7(cornell, f))
            p = frame7(cornell, f, spp)
            first = d.render_denoised(with_range(p, 0, 8), mode)
            assert not same_bits(first, want[f - 1])
            assert same_bits(d.render_denoised(with_range(p, 8, spp), mode), want[f - 1]), "frame %d, last of two passes" % f
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------------------------ 8. shards and the file key
def test_three_simulated_ranks_give_the_single_rank_frames(torch, cornell):
    mode = hjr.MODE_DENOISE
    d, r = cornell.device(), cornell.device()
    try:
        set_all(d)
        set_all(r)
        for f in range(1, 7):
            xf = moved7(cornell, f)
            d.set_transforms(*xf)
            r.set_transforms(*xf)
            p = frame7(cornell, f)
            want = d.render_denoised(p, mode)
            buf, s = render_shards(torch, r, cornell, W7, H7, SPP7, 3, True, frame=f)
            assert same_bits(r.denoise_shards(p, mode, s, W7, H7), want), "3 shards, frame %d" % f
            del buf
    finally:
        d.close()
        r.close()


def test_cli_key_writes_the_pngs_of_the_python_chain(cornell, tmp_path):
    """henjou_cli, Render_mode Denoise, 4 spp, frames 1..6 with "denoise_temporal", "denoise_variance_spatial" and "denoise_temporal_moments":
    the PNGs of the context option driven from Python, single process and through the rank path as a world of one; without the new key
    frames 1..3 are the same files and a later one is not."""
    assert os.path.exists(CLI), "henjou_cli is not built"
    work = tmp_path / "run"
    shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Image"].update(image_width=W7, image_height=H7, max_spp=SPP7)
    ro["Animation"].update(start_frame=1, end_frame=7)
    ro["Render_mode"] = "Denoise"

    def run(name, section, args=()):
        ro["Image"]["image_name"] = name
        ro["Henjou_HIP"] = section
        (work / "render_option.json").write_text(json.dumps(ro))
        q = subprocess.run([CLI, "render_option.json"] + list(args), cwd=work, capture_output=True, text=True, timeout=120, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
        assert q.returncode == 0, q.stdout + q.stderr
        return [work / ("%s_%03d.png" % (name, f)) for f in range(1, 7)]
    base = {"denoise_temporal": True, "denoise_variance_spatial": True}
    files = run("mom", dict(base, denoise_temporal_moments=True))
    d = hjr.Device(0)
    try:
        d.upload_scene(cornell.scene.view)
        set_all(d)
        for f in range(1, 7):
            t = f32_time(f, cornell.opt.fps)
            d.set_transforms(*cornell.scene.transforms(t))
            p = hjr.make_params(W7, H7, SPP7, cornell.scene.camera(cornell.opt, t), frame=f, seed=cornell.opt.seed, integrator=cornell.opt.integrator, **sky(cornell))
            want = hjr.float4_to_srgb8(d.render_denoised(p, hjr.MODE_DENOISE))[::-1]
            assert np.array_equal(hjr.load_png(str(files[f - 1])), want), "frame %d" % f
    finally:
        d.close()
    single = [p.read_bytes() for p in files]
    assert [p.read_bytes() for p in run("rank", dict(base, denoise_temporal_moments=True), ["--rank", "0", "--world", "1"])] == single
    off = [p.read_bytes() for p in run("off", dict(base, denoise_temporal_moments=False))]
    assert off[:3] == single[:3] and off[3:] != single[3:]


# ------------------------------------------------------------------------------------------------------------------ 9. the point
QW, QH, REF_SPP, QFRAMES = 96, 64, 4096, 8
_quality = {}


def quality_frames(cornell, dev, seq):
    """References (4096 spp, seed 7) and G-buffers of the eight frames of a sequence, rendered once and shared by the three sample counts."""
    if seq not in _quality:
        cam = camera_at(cornell, x=3.5)
        refs, sides = [], []
        try:
            for f in range(1, QFRAMES + 1):
                xf = moved_consistent(cornell.arrays, f if seq == "moving" else 0)
                if seq == "moving" or f == 1:
                    dev.set_transforms(*xf)
                    ref = dev.render(hjr.make_params(QW, QH, REF_SPP, cam, seed=7, **sky(cornell)), want_aovs=False)[0]
                    g = dev.gbuffer(hjr.make_params(QW, QH, 1, cam))
                refs.append(ref)
                sides.append({"camera": cam, "transforms": xf[0], "inv_transforms": xf[1], "gbuffer": g})
        finally:
            dev.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
        _quality[seq] = (refs, sides)
    return _quality[seq]


@pytest.mark.parametrize("spp", [4, 8, 1])
@pytest.mark.parametrize("seq", ["static", "moving"])
def test_quality(cornell, dev, seq, spp):
    """The point of the option.  96 x 64, NEE, seed 1, camera at x = 3.5, frames 1..8 with `frame` advancing, static and with every instance
    moved by frame * (0.05, -0.03, 0.02); references of 4096 spp with seed 7; the mask of temporal_util.ref_mask.  Frames from the GPU (the
    oracle's bits), every stage a CPU checker, so this is the table of tools/temporal_moments_rehearsal.py.  Asserted:
      static, 4 and 8 spp: moments behind the spatial estimate below the spatial estimate alone at every frame 4..8 (rehearsed margins: at
        least 8 % at 4 spp, 2.3 % at 8 spp), and moments alone below the "unknown" chain at every frame 5..8 (rehearsed: less than half);
      moving, 4 and 8 spp: mean over frames 5..8 at most 1.02 x that without moments (rehearsed 1.001 and 0.987): a cap against a
        regression, not a claimed gain.
    1 spp and the per-frame moving figures are printed, not asserted."""
    refs, sides = quality_frames(cornell, dev, seq)
    cam = sides[0]["camera"]
    frames = []
    try:
        for f, side in enumerate(sides, 1):
            dev.set_transforms(side["transforms"], side["inv_transforms"])
            c, a, n, v = dev.render(hjr.make_params(QW, QH, spp, cam, frame=f, seed=1, **sky(cornell)), want_variance=True)
            assert (v == UNKNOWN).all()
            frames.append(dict(side, color=c, albedo=a, normal=n, variance=v))
    finally:
        dev.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
    nt = n_tris(cornell)
    tables = {(seq, spp): quality_chain(frames, refs, lambda prev, cur, moments: temporal_moments_ref(prev, cur, nt, moments=moments),
                                        lambda c, a, n, v: spatial_var_ref(c, a, n, v), lambda c, a, n, v: denoise_var_ref(1, c, a, n, v)[0])}
    print(format_tables(tables))
    failed = []
    for text, holds in quality_conditions(tables):
        print("%s: %s" % (text, "holds" if holds else "FAILS"))
        if not holds:
            failed.append(text)
    assert not failed, "; ".join(failed)
