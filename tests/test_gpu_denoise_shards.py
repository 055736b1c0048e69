"""Denoise modes on the multi-GPU path (DESIGN.md §7 "Denoise modes"): hjr_assemble_shards_device against the host form, and
hjr_denoise_shards_device (rank 0's half of a frame: assemble the gathered shards, accumulate, filter, upscale) against hjr_render_denoised
on emulated ranks: one context renders every rank's share in turn, HJR_FLAG_PACKED, into slices of one torch buffer laid out as the frame's
gather leaves it.  Every comparison is bit for bit: the sharded path only moves data."""
import ctypes as C

import numpy as np
import pytest

from scene_util import Cornell, hjr
from temporal_util import moved_consistent
from test_denoise_shards_host import AOVS, SENTINEL, assemble_raw, gathered, new_outputs
from test_gpu_progressive import bits, with_range

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, SPP = 75, 41, 20  # ragged: 10 x 6 tiles; two full 8-sample chunks, so the variance is known
MODES = {"Denoise": hjr.MODE_DENOISE, "DenoiseUpScale2X": hjr.MODE_DENOISE_UPSCALE2X}
FILTERS = {"plain": (0, 0), "variance": (1, 0), "temporal": (0, 1)}  # options "denoise_variance", "denoise_temporal"
ERR_ARG, ERR_STATE = -1, -5


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def ranks(cornell):
    """The context that plays every rank in turn, and rank 0's half (hjr_denoise_shards_device) after them."""
    d = cornell.device()
    yield d
    d.close()


@pytest.fixture(scope="module")
def single(cornell):
    """The context of the single-GPU path (hjr_render_denoised): the expected frames."""
    d = cornell.device()
    yield d
    d.close()


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    same = bits(got) == bits(want)
    assert same.all(), "%s: %d of %d values differ" % (what, int((~same).sum()), same.size)


def set_filter(d, name):
    var, tmp = FILTERS[name]
    d.set_option("denoise_variance", var)
    d.set_option("denoise_temporal", tmp)  # (setting it drops the history)


def render_size(mode, w=W, h=H):
    return (w // 2, h // 2) if mode == hjr.MODE_DENOISE_UPSCALE2X else (w, h)


def render_shards(torch, dev, cornell, w, h, spp, n, variance, bounds=None, stop=None, **kw):
    """Emulated ranks: rank r's packed AOVs rendered by `dev` into slice r of one NaN-filled device buffer laid out colour | albedo | normal
    | variance per rank; ranks that own no tile are skipped.  `bounds`: sample passes; `stop(dev)`: ends a rank's passes early (adaptive)."""
    off, stride = hjr.shards_layout(w, h, n, variance=variance)
    buf = torch.full((stride * n // 4,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for r in range(n):
        if hjr.owned_tiles(w, h, r, n) == 0:
            continue
        base = buf.data_ptr() + r * stride
        p = cornell.hjr_params(w, h, spp, rank=r, world_size=n, flags=hjr.FLAG_PACKED, **kw)
        for b, e in bounds or [(0, 0)]:
            dev.render_device(with_range(p, b, e), base + off["color"], base + off["albedo"], base + off["normal"],
                              d_variance=base + off["variance"] if variance else None)
            if stop is not None and stop(dev):
                break
    return buf, hjr.make_shards(buf.data_ptr(), n, stride, off)


# ------------------------------------------------------------------------------------------------------------------ 1. device assemble
@pytest.mark.parametrize("w,h,n", [(75, 41, 1), (75, 41, 3), (75, 41, 61), (64, 64, 8)])
def test_device_assemble_equals_host_form(torch, ranks, w, h, n):
    buf, off, stride, _, _ = gathered(w, h, n)  # NaN wherever a pixel is not
    s = hjr.make_shards(buf.ctypes.data, n, stride, off)
    want = new_outputs(w, h, AOVS)
    assert assemble_raw(s, w, h, want) == 0
    d_buf = torch.from_numpy(buf).cuda()
    for present in (AOVS, ("color",), ("variance",), ("albedo", "variance")):
        outs = {k: torch.full((h, w, 4) if k != "variance" else (h, w), float(SENTINEL), dtype=torch.float32, device="cuda") for k in present}
        torch.cuda.synchronize()
        ds = hjr.make_shards(d_buf.data_ptr(), n, stride, {k: off[k] for k in present})
        ranks.assemble_shards_device(ds, w, h, **{"d_" + k: outs[k].data_ptr() for k in present})
        ranks.synchronize()
        for k in present:
            got = outs[k].cpu().numpy()
            assert not np.isnan(got).any() and not (got == SENTINEL).any(), (present, k)
            assert_bits(got, want[AOVS.index(k)], "%s of %s" % (k, present))
    # the argument rule is the host form's: an output without its source
    o = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    ds = hjr.make_shards(d_buf.data_ptr(), n, stride, {"color": off["color"]})
    rc = hjr.lib().hjr_assemble_shards_device(ranks._h, C.byref(ds), w, h, C.c_void_p(o.data_ptr()), C.c_void_p(o.data_ptr()), None, None, None)
    assert rc == ERR_ARG


# ------------------------------------------------------------------------------------------------------------------ 2. emulated ranks
@pytest.fixture(scope="module")
def expected(cornell, single):
    """(mode, filter, integrator) -> the hjr_render_denoised frame (a first frame: no history), computed once."""
    cache = {}

    def get(mode, filt, integrator=hjr.INTEGRATOR_NEE):
        key = (mode, filt, integrator)
        if key not in cache:
            set_filter(single, filt)
            rw, rh = render_size(MODES[mode])
            cache[key] = single.render_denoised(cornell.hjr_params(rw, rh, SPP, integrator=integrator), MODES[mode], W, H)
            set_filter(single, "plain")
        return cache[key]
    return get


def shards_frame(torch, ranks, cornell, mode, filt, n, integrator=hjr.INTEGRATOR_NEE, bounds=None):
    rw, rh = render_size(MODES[mode])
    set_filter(ranks, filt)
    try:
        buf, s = render_shards(torch, ranks, cornell, rw, rh, SPP, n, filt != "plain", bounds=bounds, integrator=integrator)
        return ranks.denoise_shards(cornell.hjr_params(rw, rh, SPP, integrator=integrator), MODES[mode], s, W, H)
    finally:
        set_filter(ranks, "plain")


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("mode", list(MODES))
def test_emulated_ranks_equal_render_denoised(torch, cornell, ranks, expected, mode, filt, n):
    got = shards_frame(torch, ranks, cornell, mode, filt, n)
    assert got.shape == (H, W, 4)
    assert_bits(got, expected(mode, filt), "%s, %s, %d ranks" % (mode, filt, n))


def test_emulated_ranks_more_ranks_than_tiles(torch, cornell, ranks, expected):
    """61 ranks for 60 tiles: rank 60 owns nothing, renders nothing and its block is never read."""
    assert hjr.owned_tiles(W, H, 60, 61) == 0
    assert_bits(shards_frame(torch, ranks, cornell, "Denoise", "variance", 61), expected("Denoise", "variance"), "Denoise, variance, 61 ranks")


def test_emulated_ranks_mis_integrator(torch, cornell, ranks, expected):
    """The wavefront kernel family's packed AOVs."""
    got = shards_frame(torch, ranks, cornell, "Denoise", "variance", 3, integrator=hjr.INTEGRATOR_MIS)
    assert_bits(got, expected("Denoise", "variance", hjr.INTEGRATOR_MIS), "MIS, 3 ranks")
    assert not np.array_equal(got, expected("Denoise", "variance"))


def test_filters_differ(expected):
    """The cases above are not vacuous: the three filters and the two modes give different frames."""
    frames = [expected(m, f) for m in MODES for f in FILTERS if f != "temporal"]
    for i in range(len(frames)):
        for j in range(i):
            assert not np.array_equal(frames[i], frames[j])


def test_sample_passes_gather_after_the_last(torch, cornell, ranks, expected):
    """Every rank renders the frame in 2 sample passes into its slice; the gather follows the last pass."""
    bounds = hjr.pass_bounds(SPP, 2)
    assert bounds == [(0, 8), (8, 20)]
    for filt in ("plain", "variance"):
        assert_bits(shards_frame(torch, ranks, cornell, "Denoise", filt, 3, bounds=bounds), expected("Denoise", filt), "2 passes, " + filt)


# ------------------------------------------------------------------------------------------------------------------ 3. temporal sequence
def test_temporal_sequence(torch, cornell):
    """Frames with `frame` advancing and the instances moved: hjr_denoise_shards_device at 3 ranks on one context, hjr_render_denoised on
    another; equal on every frame, so the history commits exactly once per frame on both sides.  After temporal_reset the frames are given
    in two sample passes per rank with a gather and a hjr_denoise_shards_device call after EACH pass: the call of the first pass reads the
    history and must not advance it, the call of the pass that ends at spp commits."""
    mode, n = hjr.MODE_DENOISE, 3
    a, b = cornell.device(), cornell.device()
    try:
        for d in (a, b):
            d.set_option("denoise_temporal", 1)
        first = {}
        for f in (1, 2, 3):
            xf = moved_consistent(cornell.arrays, f)
            a.set_transforms(*xf)
            b.set_transforms(*xf)
            want = b.render_denoised(cornell.hjr_params(W, H, SPP, frame=f), mode)
            buf, s = render_shards(torch, a, cornell, W, H, SPP, n, True, frame=f)
            assert_bits(a.denoise_shards(cornell.hjr_params(W, H, SPP, frame=f), mode, s), want, "frame %d" % f)
            first[f] = want
        a.temporal_reset()
        b.temporal_reset()
        for f in (2, 3, 4):
            xf = moved_consistent(cornell.arrays, f)
            a.set_transforms(*xf)
            b.set_transforms(*xf)
            p = cornell.hjr_params(W, H, SPP, frame=f)
            want = b.render_denoised(p, mode)
            if f == 2:
                assert not np.array_equal(want, first[2]), "the reset dropped the history"
            if f == 3:
                assert not np.array_equal(want, first[3]), "frame 3 after (2) differs from frame 3 after (1, 2): the history matters"
            buf, s = render_shards(torch, a, cornell, W, H, SPP, n, True, bounds=[(0, 8)], frame=f)
            preview = a.denoise_shards(with_range(p, 0, 8), mode, s)  # does not advance the history
            assert not np.array_equal(preview, want)
            # (the ranks' progressive frames ended with render_shards: render both passes again, gather after the last)
            buf, s = render_shards(torch, a, cornell, W, H, SPP, n, True, bounds=[(0, 8), (8, SPP)], frame=f)
            assert_bits(a.denoise_shards(with_range(p, 8, SPP), mode, s), want, "frame %d after the reset, last of two passes" % f)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------------------------ 4. adaptive sampling
def test_adaptive_shards(torch, cornell):
    """96 x 64, 64 spp in 4 passes, a threshold that stops some tiles and not all (tests/test_gpu_adaptive.py's: 0.1, min_samples 32): every
    rank of 3 stops its own tiles; the gathered shards through the variance-guided filter equal the single-rank adaptive frame's AOVs through
    Device.denoise(..., variance=v)."""
    w, h, spp, passes, thr, min_samples, n = 96, 64, 64, 4, 0.1, 32, 3
    bounds = hjr.pass_bounds(spp, passes)
    assert bounds == [(0, 16), (16, 32), (32, 48), (48, 64)]
    a, b = cornell.device(), cornell.device()
    try:
        b.set_adaptive(thr, min_samples)
        end, c, al, nr, v = list(b.render_adaptive(cornell.hjr_params(w, h, spp), passes, want_variance=True))[-1]
        n_tile = b.tile_samples()
        stopped = int((n_tile < spp).sum())
        print("adaptive precondition: %d of %d tiles stopped before %d spp (last pass ended at %d)" % (stopped, n_tile.size, spp, end))
        assert 1 <= stopped <= n_tile.size - 1, "the threshold must stop some tiles and not all"
        want = b.denoise(hjr.MODE_DENOISE, c, al, nr, variance=v)
        a.set_adaptive(thr, min_samples)
        a.set_option("denoise_variance", 1)
        buf, s = render_shards(torch, a, cornell, w, h, spp, n, True, bounds=bounds, stop=lambda d: d.adaptive_state()["active_tiles"] == 0)
        assert_bits(a.denoise_shards(cornell.hjr_params(w, h, spp), hjr.MODE_DENOISE, s), want, "adaptive, 3 ranks")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_enqueue_nothing_and_the_next_call_succeeds(torch, cornell, expected):
    L = hjr.lib()
    d = hjr.Device(0)
    try:
        d.upload_scene(cornell.scene.view)  # no transforms yet: no frame data
        ready = cornell.device()
        try:
            buf, s = render_shards(torch, ready, cornell, W, H, SPP, 3, True)
            ready.synchronize()
        finally:
            ready.close()
        out = torch.full((H, W, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        p = cornell.hjr_params(W, H, SPP)

        def call(mode, shards, ow=W, oh=H):
            rc = L.hjr_denoise_shards_device(d._h, C.byref(p), mode, C.byref(shards), C.c_void_p(out.data_ptr()), ow, oh, None)
            d.synchronize()
            return rc, L.hjr_last_error().decode()

        def untouched():
            return bool((out == float(SENTINEL)).all().item())
        rc, msg = call(hjr.MODE_DEFAULT, s)
        assert rc == ERR_ARG and "Default" in msg and untouched()
        d.set_option("denoise_variance", 1)
        no_var = hjr.Shards.from_buffer_copy(s)
        no_var.variance = None
        rc, msg = call(hjr.MODE_DENOISE, no_var)
        assert rc == ERR_ARG and "variance" in msg and untouched()
        no_guides = hjr.Shards.from_buffer_copy(s)
        no_guides.albedo = None
        assert call(hjr.MODE_DENOISE, no_guides)[0] == ERR_ARG and untouched()
        assert call(hjr.MODE_DENOISE, s, W + 1, H)[0] == ERR_ARG and untouched()  # Denoise: output size == render size
        assert call(7, s)[0] == ERR_ARG and untouched()
        d.set_option("denoise_variance", 0)
        d.set_option("denoise_temporal", 1)
        rc, msg = call(hjr.MODE_DENOISE, s)
        assert rc == ERR_STATE and "frame data" in msg and untouched()
        # the next valid call on the same context: its first temporal frame
        d.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
        rc, msg = call(hjr.MODE_DENOISE, s)
        assert rc == 0, msg
        assert_bits(out.cpu().numpy(), expected("Denoise", "temporal"), "the call after the refusals")
    finally:
        d.close()
