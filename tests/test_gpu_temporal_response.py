"""The windowed change test of the temporal accumulation on the GPU (hjr_temporal_accumulate_response[_device], option
"denoise_temporal_response"; csrc/hjr_temporal.hip.h section RESPONSE).  Every comparison of the kernel is GPU == the
native checker tests/native/temporal_response_ref.cpp, bit for bit on colour, variance, history, lambda and (with them) the moments; then
the ABI rules, the context option against the stateless pieces chained by hand, shards and the file key, and the quality comparison the
option is for.

Shapes: the kernel's workgroup owns 16 x 16 pixels and stages a halo of 2, so 37 x 19 has ragged tiles on both axes and windows that span
four workgroups; the rendered chains run at 48 x 32, 16 spp (two chunks: the rendered variance is known); section 5b runs every form of
the kernel through both entries at 43 x 29, 4 spp."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from denoise_var_util import denoise_var_ref
from scene_util import ROOT, Cornell, f32_time, hjr
from temporal_cov_util import mixed
from temporal_response_util import (P_TRIS, PH, PW, QFRAMES, check_planes_lambda, format_tables, geometry_changes, planes_case, quality_chain, quality_conditions,
                                    sequence_transforms, staging_case, temporal_response_ref, worst_pixels)
from temporal_util import MISS, assert_same, camera_at, moved_consistent, next_prev, ref_mask, same_bits
from test_gpu_denoise_shards import render_shards
from test_gpu_progressive import with_range

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
f32 = np.float32
ERR_ARG = -1
UNKNOWN = f32(1e30)
OPTIONS = ("denoise_temporal", "denoise_temporal_response")


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


def checked(dev, prev, cur, nt, what, moments=False):
    """Device.temporal_accumulate(response=True) == the checker on every output; returns them."""
    got = dev.temporal_accumulate(prev, cur, moments=moments, response=True)
    assert len(got) == (5 if moments else 4) and got[-1].shape == got[1].shape
    assert_same(got, temporal_response_ref(prev, cur, nt, moments=moments), what, moments)
    return got


def rendered(cornell, dev, w, h, cam, frame, xf, coverage=0, spp=16):
    """A rendered frame as the temporal stage sees it: colour, the variance AOV, the G-buffer, under the transforms xf."""
    dev.set_transforms(*xf)
    p = hjr.make_params(w, h, spp, cam, frame=frame, seed=1, **sky(cornell))
    c, a, n, v = dev.render(p, want_variance=True)
    cur = {"camera": cam, "transforms": xf[0], "inv_transforms": xf[1], "gbuffer": dev.gbuffer(p, coverage=coverage), "color": c, "variance": v}
    if coverage:
        cur["coverage"] = coverage
    return cur


def with_moments(prev, seed=3):
    h, w = prev["gbuffer"].shape
    return dict(prev, moments=np.random.default_rng(seed).uniform(0.1, 0.9, (h, w, 2)).astype(f32))


# ------------------------------------------------------------------------------------------------------------------ 1. no previous frame
def test_no_previous_frame(cornell, dev):
    """37 x 19, ragged tiles on both axes: every pixel restarts, lambda = 0, the other outputs are the plain call's."""
    cur = rendered(cornell, dev, PW, PH, camera_at(cornell), 1, moved_consistent(cornell.arrays, 0))
    assert (cur["gbuffer"]["prim"] == MISS).any() and (cur["gbuffer"]["prim"] != MISS).any()
    for moments in (False, True):
        got = checked(dev, None, cur, n_tris(cornell), "no previous frame", moments)
        assert_same(got[:-1] + (got[-1],), dev.temporal_accumulate(None, cur, moments=moments) + (np.zeros((PH, PW), f32),), "against the plain call", moments)
        assert (got[2] == 1).all() and same_bits(got[0], cur["color"])


# ------------------------------------------------------------------------------------------------------------------ 2. vacuity, then the planes
@pytest.mark.parametrize("coverage", [0, 2])
@pytest.mark.parametrize("moments", [False, True])
def test_lambda_zero_gives_the_bits_of_the_moments_call(cornell, dev, coverage, moments):
    """The same frame accumulated onto itself (identical samples: lambda = 0 everywhere) gives the bits of hjr_temporal_accumulate_moments
    in all four forms of the kernel, on a rendered 48 x 32 frame with hits, misses and (with coverage) mixed pixels.  The planes case below
    differs from its plain call: this one is not vacuous."""
    cam = camera_at(cornell, x=3.5)
    cur = rendered(cornell, dev, 48, 32, cam, 1, moved_consistent(cornell.arrays, 0), coverage=coverage)
    if coverage:
        assert mixed(cur["gbuffer"]).sum() >= 20
    prev = dict(cur, history=np.full((32, 48), 3.0, f32))
    if moments:
        prev = with_moments(prev)
    got = checked(dev, prev, cur, n_tris(cornell), "vacuity", moments)
    assert (got[-1] == 0).all() and (got[2] > 1).sum() >= 500
    assert_same(got[:-1] + (got[-1],), dev.temporal_accumulate(prev, cur, moments=moments) + (np.zeros((32, 48), f32),), "lambda = 0: the plain bits", moments)


def test_synthetic_planes(dev):
    """tests/temporal_response_util.planes_case at 37 x 19: lambda = 1 in the raised instance's interior and 0 on the right, the partial
    column beside the split, windows cut by the image's edge, an island of four pixels (too few) and one of five, a miss block."""
    prev, cur, _ = planes_case()
    for moments in (False, True):
        p = with_moments(prev) if moments else prev
        got = checked(dev, p, cur, P_TRIS, "planes", moments)
        check_planes_lambda(got[-1], "GPU")
        plain = dev.temporal_accumulate(p, cur, moments=moments)
        assert not same_bits(got[0], plain[0]) and not same_bits(got[2], plain[2])
        zero = got[-1] == 0
        assert all(same_bits(a[zero], b[zero]) for a, b in zip(got[:-1], plain)), "where lambda = 0 the outputs are the plain call's"


def test_host_entry_staging_at_an_odd_pixel_count(dev):
    """hjr_temporal_accumulate_response through its host entry point at 7 x 5 pixels, 3 instances, a previous frame, moments and response on:
    all five outputs equal tests/native/temporal_response_ref.cpp bit for bit."""
    prev, cur = staging_case()
    got = checked(dev, prev, cur, P_TRIS, "7 x 5, 3 instances", moments=True)
    assert len(got) == 5 and (got[2] > 1).any(), "pixels are carried: the previous side's images were read"


# ------------------------------------------------------------------------------------------------------------------ 3. hostile input
def test_hostile_input(dev):
    """NaN / Inf / huge colours on both sides, a NaN and an infinite history, out-of-range prim and instance ids in both G-buffers, the
    "unknown" variance, hostile moments: the call returns, equals the checker, lambda is finite and in [0, 1], a window with a NaN answers
    with 0, records with bad ids restart with lambda 0."""
    prev, cur, _ = planes_case(seed=2)
    cur["color"][3, 3, 0] = np.nan; cur["color"][5, 6, 1] = np.inf; cur["color"][9, 4, 2] = -np.inf; cur["color"][12, 8, 0] = 3e38; cur["color"][14, 25, 0] = -3e38
    prev["color"][15, 10, 1] = np.nan; prev["color"][16, 30, 0] = np.inf; prev["color"][8, 22, 2] = 3e38
    prev["history"][6, 12] = np.nan; prev["history"][6, 14] = np.inf; prev["history"][6, 16] = -np.inf
    prev["variance"][2, 2] = UNKNOWN; prev["variance"][2, 20] = np.nan; cur["variance"][7, 7] = np.nan; cur["variance"][7, 21] = UNKNOWN
    for d in (prev, cur):
        g = d["gbuffer"]
        g["prim"][17, 5] = 0xfffffffe; g["prim"][17, 7] = 1 << 30; g["inst"][17, 9] = 4; g["inst"][17, 11] = 0xffffffff; g["inst"][17, 13] = 0x80000000
        g["pos"][1, 24] = np.nan; g["pos"][1, 26] = [np.inf, 0, -4]; g["ng"][1, 28] = np.nan; g["ng"][1, 30] = 0
    cur["gbuffer"]["prim"][10, 30] = 1 << 30; prev["gbuffer"]["inst"][11, 24] = 0xffffffff
    for moments in (False, True):
        p = prev
        if moments:
            p = with_moments(prev)
            p["moments"][4, 8:14] = np.array([np.nan, np.inf, -np.inf, 1e38, 3e38, -4.0], f32)[:, None]
        got = checked(dev, p, cur, P_TRIS, "hostile", moments)
        lam = got[-1]
        assert np.isfinite(lam).all() and (lam >= 0).all() and (lam <= 1).all()
        assert (lam[1:6, 1:6] == 0).all(), "a NaN in the window: t is NaN"
        for y, x in ((17, 5), (17, 7), (17, 9), (17, 11), (17, 13), (10, 30)):
            assert lam[y, x] == 0 and got[2][y, x] == 1 and same_bits(got[0][y, x], cur["color"][y, x])


# ------------------------------------------------------------------------------------------------------------------ 4. rendered chains
def test_light_chain(cornell, dev):
    """Sequence L at 48 x 32 x 16 spp, frames 3 -> 4 -> 5 (the light stands at 3 and has moved at 4 and 5), from a two-frame history: the
    change test answers at frames 4 and 5 and hardly at frame 3."""
    cam = camera_at(cornell, x=3.5)
    prev, share = None, {}
    try:
        for f in range(1, 6):
            cur = rendered(cornell, dev, 48, 32, cam, f, sequence_transforms(cornell.arrays, "L", f))
            got = checked(dev, prev, cur, n_tris(cornell), "L, frame %d" % f)
            share[f] = float((got[3] > 0).mean())
            prev = next_prev(cur, got)
    finally:
        dev.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
    print("share of pixels with lambda > 0 per frame:", share)
    assert share[1] == 0 and share[3] < share[4] < share[5]  # (the CPU rehearsal at this size: 10.5 %, 21.5 %, 37.1 %)


@pytest.mark.parametrize("form", ["plain", "coverage4", "moments"])
def test_moving_chain_with_a_turning_camera(cornell, dev, form):
    """Sequence M with the camera turned and shifted a little more each frame, 48 x 32 x 16 spp, four frames: the window runs over
    bilinearly reprojected history, restarted pixels are no members.  Also with the coverage G-buffer of side 4 and with the moments."""
    coverage, moments = (4 if form == "coverage4" else 0), form == "moments"
    prev, fractional = None, 0
    try:
        for f in range(1, 5):
            cam = camera_at(cornell, x=3.5, turn=0.03 * f, shift=(-0.072 * f, 0.048 * f, 0.09 * f))
            cur = rendered(cornell, dev, 48, 32, cam, f, moved_consistent(cornell.arrays, f), coverage=coverage)
            got = checked(dev, prev, cur, n_tris(cornell), "M (%s), frame %d" % (form, f), moments)
            hh = got[2]
            fractional += int(((hh > 1) & (np.abs(hh - np.round(hh)) > 1e-3)).sum())
            prev = next_prev(cur, got, moments)
            if coverage:
                prev["coverage"] = coverage
    finally:
        dev.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
    assert fractional >= 1 and (got[-1] > 0).any() and (got[-1] == 0).any() and (got[2] == 1).any()


# ------------------------------------------------------------------------------------------------------------------ 5. ABI
def raw_call(dev, prev, cur, prev_moments, out_moments, out_response, frame_size=None, fill=7.0):
    """hjr_temporal_accumulate_response on sentinel-filled outputs: (status, colour, variance, history, moments or None, lambda or None)."""
    keep = []
    fc = hjr.Device._temporal_frame(cur, keep)
    fp = None if prev is None else hjr.Device._temporal_frame(prev, keep)
    for f in (fc, fp):
        if f is not None and frame_size is not None:
            f.struct_size = frame_size
    h, w = fc.height, fc.width
    outs = [np.full((h, w, 4), fill, f32), np.full((h, w), fill, f32), np.full((h, w), fill, f32), np.full((h, w, 2), fill, f32) if out_moments else None,
            np.full((h, w), fill, f32) if out_response else None]
    pm = None if prev_moments is None else np.ascontiguousarray(prev_moments, f32)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = hjr.lib().hjr_temporal_accumulate_response(dev._h, None if fp is None else C.byref(fp), C.byref(fc), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(pm), ptr(outs[3]),
                                                    ptr(outs[4]))
    return (rc,) + tuple(outs)


def test_abi_rules(torch, dev):
    """out_response == NULL is hjr_temporal_accumulate_moments bit for bit (and hjr_temporal_accumulate with out_moments NULL as well);
    out_moments with a previous frame and no prev_moments stays HJR_ERR_ARG and writes nothing; 128- and 124-byte frames work; the device
    form gives the host form's bits."""
    prev, cur, _ = planes_case()
    prev = with_moments(prev)
    plain, plain_m = dev.temporal_accumulate(prev, cur), dev.temporal_accumulate(prev, cur, moments=True)
    want, want_m = dev.temporal_accumulate(prev, cur, response=True), dev.temporal_accumulate(prev, cur, moments=True, response=True)
    assert C.sizeof(hjr.TemporalFrame) == 128
    rc, c, v, h, m, lam = raw_call(dev, prev, cur, prev["moments"], True, False)
    assert rc == 0
    assert_same((c, v, h, m, m), plain_m + (plain_m[3],), "out_response == NULL", True)
    rc, c, v, h, m, lam = raw_call(dev, prev, cur, None, False, False)
    assert rc == 0
    assert_same((c, v, h, h), plain + (plain[2],), "both NULL")
    rc, c, v, h, m, lam = raw_call(dev, prev, cur, None, True, True)
    assert rc == ERR_ARG and b"moments" in hjr.lib().hjr_last_error()
    assert all((a == 7).all() for a in (c, v, h, m, lam)), "nothing was enqueued"
    rc, *got = raw_call(dev, prev, cur, np.full((PH, PW, 2), np.nan, f32), False, True)  # without moments prev_moments is not looked at
    assert rc == 0
    assert_same((got[0], got[1], got[2], got[4]), want, "response without moments")
    for size in (128, 124):
        rc, *got = raw_call(dev, prev, cur, prev["moments"], True, True, size)
        assert rc == 0
        assert_same(got, want_m, "%d-byte frames" % size, True)
    # the device form
    keep, t = [], {}
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
    d_out = [torch.full(s, 7.0, dtype=torch.float32, device="cuda") for s in ((PH, PW, 4), (PH, PW), (PH, PW), (PH, PW, 2), (PH, PW))]
    torch.cuda.synchronize()
    L = hjr.lib()
    ptr = lambda a: C.c_void_p(a.data_ptr())
    assert L.hjr_temporal_accumulate_response_device(dev._h, C.byref(dp), C.byref(dc), ptr(d_out[0]), ptr(d_out[1]), ptr(d_out[2]), ptr(t["pmoments"]), ptr(d_out[3]),
                                                     ptr(d_out[4]), None) == 0
    dev.synchronize()
    assert_same([a.cpu().numpy() for a in d_out], want_m, "device form", True)
    for a in d_out:
        a.fill_(7)
    torch.cuda.synchronize()
    assert L.hjr_temporal_accumulate_response_device(dev._h, C.byref(dp), C.byref(dc), ptr(d_out[0]), ptr(d_out[1]), ptr(d_out[2]), ptr(t["pmoments"]), ptr(d_out[3]), None, None) == 0
    dev.synchronize()
    assert_same([a.cpu().numpy() for a in d_out[:4]] + [d_out[3].cpu().numpy()], plain_m + (plain_m[3],), "device form, out_response == NULL", True)
    assert (d_out[4].cpu().numpy() == 7).all()
    assert L.hjr_temporal_accumulate_response_device(dev._h, C.byref(dp), C.byref(dc), ptr(d_out[0]), ptr(d_out[1]), ptr(d_out[2]), None, ptr(d_out[3]), ptr(d_out[4]), None) == ERR_ARG
    assert L.hjr_temporal_accumulate_response_device(dev._h, C.byref(dp), C.byref(dc), ptr(d_out[0]), ptr(d_out[1]), None, None, None, ptr(d_out[4]), None) == ERR_ARG
    dev.synchronize()
    assert (d_out[4].cpu().numpy() == 7).all(), "nothing was enqueued"


# ------------------------------------------------------------------------------------------------------------------ 5b. every form, both entries
FW, FH = 43, 29  # odd on both axes, no multiple of the response kernel's 16 x 16 tile or of the 64 x 4 grid cell, and an odd pixel count


@pytest.fixture(scope="module")
def form_frames(cornell, dev):
    """{coverage: (prev, cur)} at 43 x 29 x 4 spp: frame 1 with a history of 5 everywhere and random moments, and frame 2 with every
    instance moved one step, so the taps are bilinear and the window test has something to answer to.  Rendered once for the eight cases."""
    cam, frames = camera_at(cornell), {}
    try:
        for coverage in (0, 2):
            prev = rendered(cornell, dev, FW, FH, cam, 1, moved_consistent(cornell.arrays, 0), coverage=coverage, spp=4)
            prev = with_moments(dict(prev, history=np.full((FH, FW), 5.0, f32)))
            frames[coverage] = (prev, rendered(cornell, dev, FW, FH, cam, 2, moved_consistent(cornell.arrays, 1), coverage=coverage, spp=4))
    finally:
        dev.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
    return frames


@pytest.mark.parametrize("response", [False, True])
@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("coverage", [0, 2])
def test_every_form_host_and_device_entry(torch, cornell, dev, form_frames, coverage, moments, response):
    """All eight kernels (coverage x moments x response) at 43 x 29: the host entry, whose staging buffer then holds images of an odd
    number of pixels back to back, equals the checker bit for bit in every returned array, and the matching _device entry on torch buffers
    equals the host entry."""
    prev, cur = form_frames[coverage]
    hit = cur["gbuffer"]["prim"] != MISS
    assert hit.any() and not hit.all() and (not coverage or mixed(cur["gbuffer"]).any())
    got = dev.temporal_accumulate(prev, cur, moments=moments, response=response)
    want = temporal_response_ref(prev, cur, n_tris(cornell), moments=moments, response=response)
    assert len(got) == 3 + moments + response
    assert_same(got, want, "host entry against the checker", moments)
    assert (got[2] > 1).sum() >= 100 and (got[2] == 1).any() and (not response or (got[-1] > 0).any()), "carried pixels, restarts, a lambda above 0"
    # the device entry of the same form
    keep, t = [], {}
    for name, d in (("p", prev), ("c", cur)):
        for key in ("transforms", "inv_transforms", "color", "variance", "history", "moments"):
            if d.get(key) is not None:
                t[name + key] = torch.from_numpy(np.ascontiguousarray(d[key], f32)).cuda()
        t[name + "gbuffer"] = torch.from_numpy(np.ascontiguousarray(d["gbuffer"]).view(np.uint8).reshape(-1).copy()).cuda()
    frames = []
    for name, d in (("p", prev), ("c", cur)):
        f = hjr.Device._temporal_frame(d, keep)
        f.transforms12, f.inv_transforms12, f.gbuffer = t[name + "transforms"].data_ptr(), t[name + "inv_transforms"].data_ptr(), t[name + "gbuffer"].data_ptr()
        f.color, f.variance = t[name + "color"].data_ptr(), t[name + "variance"].data_ptr()
        f.history = t[name + "history"].data_ptr() if name == "p" else None
        frames.append(f)
    shapes = [(FH, FW, 4), (FH, FW), (FH, FW)] + ([(FH, FW, 2)] if moments else []) + ([(FH, FW)] if response else [])
    d_out = [torch.full(s, 7.0, dtype=torch.float32, device="cuda") for s in shapes]
    torch.cuda.synchronize()
    L = hjr.lib()
    ptr = lambda a: C.c_void_p(a.data_ptr())
    head = (dev._h, C.byref(frames[0]), C.byref(frames[1]), ptr(d_out[0]), ptr(d_out[1]), ptr(d_out[2]))
    mom_args = (ptr(t["pmoments"]), ptr(d_out[3])) if moments else (None, None)
    if response:
        rc = L.hjr_temporal_accumulate_response_device(*head, *mom_args, ptr(d_out[-1]), None)
    elif moments:
        rc = L.hjr_temporal_accumulate_moments_device(*head, *mom_args, None)
    else:
        rc = L.hjr_temporal_accumulate_device(*head, None)
    assert rc == 0, L.hjr_last_error()
    dev.synchronize()
    on_device = tuple(a.cpu().numpy() for a in d_out)
    assert_same(on_device, got, "device entry against the host entry", moments)


# ------------------------------------------------------------------------------------------------------------------ 6. the context option
W6, H6, SPP6, FRAMES6 = 48, 32, 16, 5


def xf6(cornell, f):
    return sequence_transforms(cornell.arrays, "L", f + 2)  # the light stands for the first frame and moves from the second on


def frame6(cornell, f, spp=SPP6):
    return cornell.hjr_params(W6, H6, spp, frame=f)


def by_hand(d, p, mode, xf, prev, response=True, moments=False, spatial=False, coverage=0):
    """render with the variance -> (3 x 3 estimate) -> G-buffer -> accumulate against `prev` -> variance-guided filter: (image, new history)."""
    c, a, n, v = d.render(p, want_variance=True)
    cur = {"camera": hjr.Camera.from_buffer_copy(p.camera), "transforms": xf[0], "inv_transforms": xf[1], "gbuffer": d.gbuffer(p, coverage=coverage), "color": c,
           "variance": d.estimate_variance(c, a, n, v) if spatial else v}
    if coverage:
        cur["coverage"] = coverage
    out = d.temporal_accumulate(prev, cur, moments=moments, response=response)
    nxt = next_prev(cur, out, moments)
    return d.denoise(mode, out[0], a, n, variance=out[1]), nxt


def hand_chain(cornell, d, mode, response=True, spp=SPP6, **kw):
    out, prev = [], None
    for f in range(1, FRAMES6 + 1):
        xf = xf6(cornell, f)
        d.set_transforms(*xf)
        img, prev = by_hand(d, frame6(cornell, f, spp), mode, xf, prev, response, **kw)
        out.append(img)
    return out


def set_all(d, keys=OPTIONS, value=1):
    for key in keys:
        d.set_option(key, value)


def test_context_chain_equals_the_pieces(cornell):
    """Five frames of hjr_render_denoised, 48 x 32, 16 spp, the light moving from the second frame on, with "denoise_temporal" and the new
    option: the stateless pieces chained by hand, bit for bit, and not the chain without the change test; setting the option drops the
    history; with the option at 0 the frames are the parent's; it composes with the moments, the spatial estimate, coverage and "firefly_clamp"."""
    mode = hjr.MODE_DENOISE
    d = cornell.device()
    try:
        want, without = hand_chain(cornell, d, mode), hand_chain(cornell, d, mode, response=False)
        assert same_bits(want[0], without[0]) and not same_bits(want[2], without[2])
        assert d.get_option("denoise_temporal_response") == -1
        set_all(d)
        assert d.get_option("denoise_temporal_response") == 1
        for f in range(1, FRAMES6 + 1):
            d.set_transforms(*xf6(cornell, f))
            assert same_bits(d.render_denoised(frame6(cornell, f), mode), want[f - 1]), "frame %d" % f
        # setting the option (to the value it has) drops the history: the last frame again is a first frame
        d.set_option("denoise_temporal_response", 1)
        first = by_hand(d, frame6(cornell, FRAMES6), mode, xf6(cornell, FRAMES6), None)[0]
        assert same_bits(d.render_denoised(frame6(cornell, FRAMES6), mode), first) and not same_bits(first, want[-1])
        # option 0: the parent's frames
        d.set_option("denoise_temporal_response", 0)
        for f in range(1, FRAMES6 + 1):
            d.set_transforms(*xf6(cornell, f))
            assert same_bits(d.render_denoised(frame6(cornell, f), mode), without[f - 1]), "option 0, frame %d" % f
        with pytest.raises(hjr.HjrError):
            d.set_option("denoise_temporal_response", 2)
        # with the moments, the spatial estimate, the coverage G-buffer and the firefly clamp
        d.set_option("firefly_clamp", 8)
        full = hand_chain(cornell, d, mode, moments=True, spatial=True, coverage=2)
        set_all(d, OPTIONS + ("denoise_temporal_moments", "denoise_variance_spatial"))
        d.set_option("denoise_temporal_coverage", 2)
        for f in range(1, FRAMES6 + 1):
            d.set_transforms(*xf6(cornell, f))
            assert same_bits(d.render_denoised(frame6(cornell, f), mode), full[f - 1]), "all options, frame %d" % f
        # without "denoise_temporal" it has no effect, and Default mode ignores it
        for key in ("denoise_temporal_moments", "denoise_variance_spatial", "denoise_temporal_coverage", "denoise_temporal"):
            d.set_option(key, 0)
        d.set_option("denoise_variance", 1)
        p = frame6(cornell, 3)
        c, a, n, v = d.render(p, want_variance=True)
        assert same_bits(d.render_denoised(p, mode), d.denoise(mode, c, a, n, variance=v))
        d.set_option("denoise_temporal", 1)
        assert same_bits(d.render_denoised(p, hjr.MODE_DEFAULT), d.render(p, want_aovs=False)[0])
    finally:
        d.close()


def test_two_sample_passes_advance_the_history_once(cornell):
    """Frames of 16 spp rendered in passes of 8 and 8 samples: the first pass accumulates and discards, the last pass ends on the one-shot
    bits."""
    mode = hjr.MODE_DENOISE_UPSCALE2X
    d = cornell.device()
    try:
        want, without = hand_chain(cornell, d, mode), hand_chain(cornell, d, mode, response=False)
        assert not same_bits(want[2], without[2])
        set_all(d)
        for f in range(1, FRAMES6 + 1):
            d.set_transforms(*xf6(cornell, f))
            p = frame6(cornell, f)
            first = d.render_denoised(with_range(p, 0, 8), mode)
            assert not same_bits(first, want[f - 1])
            assert same_bits(d.render_denoised(with_range(p, 8, SPP6), mode), want[f - 1]), "frame %d, last of two passes" % f
    finally:
        d.close()


def test_three_simulated_ranks_give_the_single_rank_frames(torch, cornell):
    mode = hjr.MODE_DENOISE
    d, r = cornell.device(), cornell.device()
    try:
        set_all(d)
        set_all(r)
        for f in range(1, FRAMES6 + 1):
            xf = xf6(cornell, f)
            d.set_transforms(*xf)
            r.set_transforms(*xf)
            p = frame6(cornell, f)
            want = d.render_denoised(p, mode)
            buf, s = render_shards(torch, r, cornell, W6, H6, SPP6, 3, True, frame=f)
            assert same_bits(r.denoise_shards(p, mode, s, W6, H6), want), "3 shards, frame %d" % f
            del buf
    finally:
        d.close()
        r.close()


def test_cli_key_writes_the_pngs_of_the_python_chain(cornell, tmp_path):
    """henjou_cli, Render_mode Denoise, 16 spp, frames 1..5 with "denoise_temporal" and "denoise_temporal_response": the PNGs of the context
    option driven from Python, single process and through the rank path as a world of one; false is the file without the key."""
    assert os.path.exists(CLI), "henjou_cli is not built"
    work = tmp_path / "run"
    shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Image"].update(image_width=W6, image_height=H6, max_spp=SPP6)
    ro["Animation"].update(start_frame=1, end_frame=6)
    ro["Render_mode"] = "Denoise"

    def run(name, section, args=()):
        ro["Image"]["image_name"] = name
        ro["Henjou_HIP"] = section
        (work / "render_option.json").write_text(json.dumps(ro))
        q = subprocess.run([CLI, "render_option.json"] + list(args), cwd=work, capture_output=True, text=True, timeout=120, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
        assert q.returncode == 0, q.stdout + q.stderr
        return [work / ("%s_%03d.png" % (name, f)) for f in range(1, 6)]
    files = run("resp", {"denoise_temporal": True, "denoise_temporal_response": True})
    d = hjr.Device(0)
    try:
        d.upload_scene(cornell.scene.view)
        set_all(d)
        for f in range(1, 6):
            t = f32_time(f, cornell.opt.fps)
            d.set_transforms(*cornell.scene.transforms(t))
            p = hjr.make_params(W6, H6, SPP6, cornell.scene.camera(cornell.opt, t), frame=f, seed=cornell.opt.seed, integrator=cornell.opt.integrator, **sky(cornell))
            want = hjr.float4_to_srgb8(d.render_denoised(p, hjr.MODE_DENOISE))[::-1]
            assert np.array_equal(hjr.load_png(str(files[f - 1])), want), "frame %d" % f
    finally:
        d.close()
    single = [p.read_bytes() for p in files]
    assert [p.read_bytes() for p in run("rank", {"denoise_temporal": True, "denoise_temporal_response": True}, ["--rank", "0", "--world", "1"])] == single
    off = [p.read_bytes() for p in run("off", {"denoise_temporal": True, "denoise_temporal_response": False})]
    assert off == [p.read_bytes() for p in run("none", {"denoise_temporal": True})]
    assert off[0] == single[0]


# ------------------------------------------------------------------------------------------------------------------ 7. the point
QSPP = 16
QSIZES = {"96x64": (96, 64, 4096), "48x32": (48, 32, 2048)}  # width, height, samples of the references
_tables = {}


def quality_table(cornell, dev, size, seq):
    """One sequence's table: frames and references from the GPU (the oracle's bits), every stage a CPU checker, so this is the table of
    tools/temporal_response_rehearsal.py.  Computed once per size and sequence."""
    if (size, seq) not in _tables:
        qw, qh, ref_spp = QSIZES[size]
        cam = camera_at(cornell, x=3.5)
        refs, frames = [], []
        try:
            for f in range(1, QFRAMES + 1):
                xf = sequence_transforms(cornell.arrays, seq, f)
                dev.set_transforms(*xf)
                if geometry_changes(seq, f):
                    ref = dev.render(hjr.make_params(qw, qh, ref_spp, cam, seed=7, **sky(cornell)), want_aovs=False)[0]
                    g = dev.gbuffer(hjr.make_params(qw, qh, 1, cam))
                refs.append(ref)
                c, a, n, v = dev.render(hjr.make_params(qw, qh, QSPP, cam, frame=f, seed=1, **sky(cornell)), want_variance=True)
                frames.append({"camera": cam, "transforms": xf[0], "inv_transforms": xf[1], "gbuffer": g, "color": c, "albedo": a, "normal": n, "variance": v})
        finally:
            dev.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
        nt = n_tris(cornell)
        t = quality_chain(frames, refs, lambda prev, cur, response: temporal_response_ref(prev, cur, nt, response=response),
                          lambda c, a, n, v: denoise_var_ref(1, c, a, n, v)[0])
        _tables[(size, seq)] = (t, refs)
    return _tables[(size, seq)]


@pytest.mark.parametrize("seq", ["S", "L", "M"])
@pytest.mark.parametrize("size", ["96x64", "48x32"])
def test_quality(cornell, dev, size, seq):
    """The point of the option.  NEE, 16 spp, seed 1, camera at x = 3.5, frames 1..10 with `frame` advancing; S static, L with only the
    light's instance moved by (0.12 max(0, f - 3), 0, 0), M with every instance moved by f * (0.05, -0.03, 0.02); references with seed 7 (4096
    spp at 96 x 64, 2048 at 48 x 32); the mask of temporal_util.ref_mask; the same renders for every column.  The tables repeat those of
    tools/temporal_response_rehearsal.py digit for digit.  Asserted:
      L: mean e_resp(4..10) < mean e_var(4..10)                                            [96 x 64: 0.04545 < 0.04678; 48 x 32: 0.05666 < 0.06084]
      S: mean e_resp(4..10) <= 1.02 x mean e_tmp(4..10)                                    [96 x 64: 0.04291, 0.04244: 1.011; 48 x 32: 1.0007]
      S: §11.2's four conditions with e_resp in place of e_tmp
      L, at 48 x 32: mean e_resp(4..10) < 0.75 x mean e_tmp(4..10);  e_resp(4) < 0.5 x e_tmp(4)   [0.05666, 0.09233: 0.61;  0.04600, 0.12853: 0.36]
    Reported, not asserted: the last two at 96 x 64.  There the plain temporal path does not lose the frames after the light moves
    (e_tmp(4) 0.04365 against e_var(4) 0.04709; mean e_tmp(4..10) 0.04604 against mean e_var 0.04678), so nothing can halve its error:
    0.04545 against 0.75 x 0.04604 and 0.04504 against 0.5 x 0.04365 with R = 2, 0.04548 and 0.04521 with the one re-tune R = 3, which is
    therefore not taken.  M is printed with the ten worst pixels of its worst frame."""
    t, refs = quality_table(cornell, dev, size, seq)
    print(format_tables({seq: t}))
    if seq == "M":
        f = int(np.argmax(t["e_resp"]))
        print("M   worst frame %d (e_resp %.5f, e_tmp %.5f)" % (f + 1, t["e_resp"][f], t["e_tmp"][f]))
        print("\n".join("M   " + s for s in worst_pixels(t["out_resp"][f], refs[f], ref_mask(refs[f]))))
    failed = []
    for text, holds, asserted in quality_conditions({seq: t}, QSIZES[size][:2]):
        print("%s: %s" % (text, "holds" if holds else "FAILS" if asserted else "fails (reported at this size)"))
        if asserted and not holds:
            failed.append(text)
    assert not failed, "; ".join(failed)
