"""The variance AOV on the GPU (hjr_render_var; include/henjou_hip.h, DESIGN.md §4 rule 7).

The expected variance is numpy float32: the oracle's per-sample values are summed into chunk sums as the render kernels sum them
(samples of a chunk in sample order from +0.0f), then rule 7 is applied (tests/denoise_var_util.py).  The GPU must give the same bits
for one-shot frames, sample passes and adaptive frames, packed or not, and the other AOVs must not notice the fourth pointer.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
from denoise_var_util import UNKNOWN, variance_rule
from scene_util import Cornell, hjr
from test_gpu_adaptive import even_bounds, oracle_chunks, owned_samples, predict
from test_gpu_progressive import SENTINEL, assert_same, bits, with_range

pytestmark = pytest.mark.gpu
ERR_STATE = -5
f32 = np.float32
W, H = 20, 12  # partial tiles in x and in y


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def dev(cornell):
    d = cornell.device()
    yield d
    d.close()


_cache = {}


def chunk_sums(cornell, w, h, spp, integ=hjr.INTEGRATOR_NEE):
    """([chunk][y][x][aov][rgb] float32, granule, full chunks): the last chunk is the partial one when spp is no multiple of the granule."""
    key = (w, h, spp, integ)
    if key not in _cache:
        g = hjr.sample_granule(spp)
        osc = ob.OracleScene(cornell.arrays, ob.MATH_PORTABLE)
        op = cornell.oracle_params(w, h, spp, integrator=integ)
        n = (spp + g - 1) // g
        chunk = np.zeros((n, h, w, 3, 3), f32)
        for y in range(h):
            for x in range(w):
                for k in range(n):
                    acc = np.zeros((3, 3), f32)
                    for s in range(g * k, min(g * k + g, spp)):
                        acc = acc + np.stack(osc.sample(op, x, y, s))
                    chunk[k, y, x] = acc
        _cache[key] = (chunk, g, spp // g)
    return _cache[key]


def mean_of(chunk, n_chunks, n):
    run = np.zeros(chunk.shape[1:], f32)
    for k in range(n_chunks):
        run = run + chunk[k]
    out = np.ones((3,) + chunk.shape[1:3] + (4,), f32)
    out[..., :3] = np.moveaxis(run * (f32(1) / f32(n)), 2, 0)
    return list(out)


def render_var(dev, p, shape, aovs=True, variance=True):
    """hjr_render_var into sentinel-filled arrays: (status, [color, albedo, normal], variance)."""
    out = [np.full(shape, SENTINEL, f32)] + [np.full(shape, SENTINEL, f32) if aovs else None for _ in range(2)]
    var = np.full(shape[:-1], SENTINEL, f32) if variance else None
    rc = hjr.lib().hjr_render_var(dev._h, C.byref(p), *[None if a is None else a.ctypes.data for a in out], None if var is None else var.ctypes.data)
    return rc, out, var


def same_bits(got, want, what):
    same = bits(got) == bits(want)
    assert same.all(), "%s: %d of %d variances differ, first got %r want %r" % (what, int((~same).sum()), same.size, got[~same][:3], want[~same][:3])


@pytest.mark.parametrize("spp", [16, 40, 44])
def test_one_shot_bits(cornell, dev, spp):
    """16 spp (m = 2, the minimum), 40 (5 full chunks), 44 (5 full chunks and a partial one, which the colour gets and the variance does
    not): variance bits; the three other AOVs equal the same call without the pointer (a NULL pointer is hjr_render) and the oracle."""
    chunk, g, n_full = chunk_sums(cornell, W, H, spp)
    assert g == 8 and n_full == spp // 8 and chunk.shape[0] == (spp + 7) // 8
    p = cornell.hjr_params(W, H, spp)
    rc, out, var = render_var(dev, p, (H, W, 4))
    assert rc == 0, hjr.lib().hjr_last_error()
    want = variance_rule(chunk[:, :, :, 0, :], g, n_full, spp)
    assert (want != UNKNOWN).all() and (want > 0).any()
    same_bits(var, want, "one-shot %d spp" % spp)
    assert_same(out, mean_of(chunk, chunk.shape[0], spp), "AOVs with the variance pointer vs the oracle's samples")
    rc, plain, none = render_var(dev, p, (H, W, 4), variance=False)
    assert rc == 0 and none is None
    assert_same(out, plain, "AOVs with and without the variance pointer")
    assert_same(out, list(dev.render(p)), "hjr_render")
    c4 = dev.render(p, want_variance=True)
    assert len(c4) == 4 and c4[3].shape == (H, W)
    same_bits(c4[3], want, "Device.render(want_variance=True)")
    rc, conly, v2 = render_var(dev, p, (H, W, 4), aovs=False)  # colour-only render kernel variant
    assert rc == 0
    same_bits(v2, want, "colour + variance only")
    assert_same(conly, [out[0], None, None], "colour of the colour-only call")


@pytest.mark.parametrize("spp", [8, 4])
def test_single_chunk_frames_are_unknown(cornell, dev, spp):
    """At most 8 spp there are no chunk sums: the fill path writes UNKNOWN to every pixel, and the AOVs are the plain call's."""
    p = cornell.hjr_params(W, H, spp)
    rc, out, var = render_var(dev, p, (H, W, 4))
    assert rc == 0, hjr.lib().hjr_last_error()
    assert (var == UNKNOWN).all()
    assert_same(out, list(dev.render(p)), "%d spp" % spp)


def test_granule_16_at_1024_spp(cornell, dev):
    chunk, g, n_full = chunk_sums(cornell, 8, 8, 1024)
    assert g == 16 and n_full == 64
    rc, out, var = render_var(dev, cornell.hjr_params(8, 8, 1024), (8, 8, 4))
    assert rc == 0, hjr.lib().hjr_last_error()
    same_bits(var, variance_rule(chunk[:, :, :, 0, :], g, n_full, 1024), "1024 spp")
    assert_same(out, mean_of(chunk, 64, 1024), "1024 spp AOVs")


def test_mis_runs_the_other_kernel_family(cornell, dev):
    chunk, g, n_full = chunk_sums(cornell, W, H, 40, hjr.INTEGRATOR_MIS)
    rc, out, var = render_var(dev, cornell.hjr_params(W, H, 40, integrator=hjr.INTEGRATOR_MIS), (H, W, 4))
    assert rc == 0, hjr.lib().hjr_last_error()
    assert dev.stats()["pipeline"] == 1  # the wavefront kernels (NEE above ran the megakernel)
    same_bits(var, variance_rule(chunk[:, :, :, 0, :], g, n_full, 40), "MIS 40 spp")
    rc, out, var = render_var(dev, cornell.hjr_params(W, H, 40), (H, W, 4))
    assert rc == 0 and dev.stats()["pipeline"] == 0


def test_sample_passes(cornell, dev):
    """40 spp as [0, 8) [8, 24) [24, 40): UNKNOWN after one granule, n = 24 after the second pass, the one-shot bits after the last.
    Dropping (or adding) the variance pointer on a continuing pass is HJR_ERR_STATE, touches nothing, and a corrected call goes on."""
    chunk, g, _ = chunk_sums(cornell, W, H, 40)
    col = chunk[:, :, :, 0, :]
    p = cornell.hjr_params(W, H, 40)
    rc, one, one_var = render_var(dev, p, (H, W, 4))
    assert rc == 0
    rc, out, var = render_var(dev, with_range(p, 0, 8), (H, W, 4))
    assert rc == 0, hjr.lib().hjr_last_error()
    assert (var == UNKNOWN).all()
    assert_same(out, mean_of(chunk, 1, 8), "pass [0, 8)")
    rc, out, var = render_var(dev, with_range(p, 8, 24), (H, W, 4), variance=False)  # the pointer dropped
    assert rc == ERR_STATE and b"AOVs" in hjr.lib().hjr_last_error()
    assert all((a == SENTINEL).all() for a in out)
    rc, out, var = render_var(dev, with_range(p, 8, 24), (H, W, 4))
    assert rc == 0, hjr.lib().hjr_last_error()
    same_bits(var, variance_rule(col, g, 3, 24), "pass [8, 24)")
    assert_same(out, mean_of(chunk, 3, 24), "pass [8, 24)")
    rc, out, var = render_var(dev, with_range(p, 24, 40), (H, W, 4))
    assert rc == 0, hjr.lib().hjr_last_error()
    same_bits(var, one_var, "last pass vs one-shot")
    assert_same(out, one, "last pass vs one-shot")
    # a frame begun without the variance cannot gain it
    rc, out, var = render_var(dev, with_range(p, 0, 16), (H, W, 4), variance=False)
    assert rc == 0
    rc, out, var = render_var(dev, with_range(p, 16, 40), (H, W, 4))
    assert rc == ERR_STATE and (var == SENTINEL).all() and all((a == SENTINEL).all() for a in out)
    # the generator form, with a partial last chunk: 44 spp in 3 passes
    chunk44, _, n_full = chunk_sums(cornell, W, H, 44)
    ends = []
    for e, c, a, n, v in dev.render_progressive(cornell.hjr_params(W, H, 44), 3, want_variance=True):
        same_bits(v, variance_rule(chunk44[:, :, :, 0, :], 8, e // 8, e), "render_progressive sample_end %d" % e)
        ends.append(e)
    assert ends == [8, 24, 44]


def test_adaptive_frame(cornell):
    """48 x 32, 128 spp in passes of 16, threshold 0.1, min_samples 32 (a case of tests/test_gpu_adaptive.py): some tiles stop, others stay
    active to the end.  After every pass a stopped tile's variance is the one over its n_tile samples (so it stays put), an active tile's
    is over sample_end; the AOVs are those of the adaptive frame without the pointer."""
    w, h, spp, step, thr = 48, 32, 128, 16, 0.1
    bounds = even_bounds(spp, step)
    chunk = oracle_chunks(cornell, w, h, spp, hjr.INTEGRATOR_NEE)
    pred = predict(chunk, w, h, spp, bounds, thr, 32)
    last = pred[-1][0]
    assert (last < spp).any() and (last == spp).any(), "the threshold must stop some tiles and leave others active"
    dev = cornell.device()
    dev.set_adaptive(thr, 32)
    p = cornell.hjr_params(w, h, spp)
    prev = None
    for (b, e), (n_tile, want, active) in zip(bounds, pred):
        rc, out, var = render_var(dev, with_range(p, b, e), (h, w, 4))
        assert rc == 0, hjr.lib().hjr_last_error()
        assert dev.adaptive_state()["active_tiles"] == active
        assert_same(out, want, "adaptive pass [%d, %d)" % (b, e))
        n_px = np.kron(n_tile, np.ones((8, 8), np.uint32))[:h, :w]
        exp = np.zeros((h, w), f32)
        for n in np.unique(n_px):
            v = variance_rule(chunk[:, :, :, 0, :], 8, int(n) // 8, int(n))
            exp = np.where(n_px == n, v, exp)
        same_bits(var, exp, "adaptive pass [%d, %d)" % (b, e))
        if prev is not None:
            stopped = n_px < b  # stopped before this pass began
            if stopped.any():
                assert np.array_equal(bits(var)[stopped], bits(prev)[stopped]), "a stopped tile's variance moved"
        prev = var
    dev.close()


def test_adaptive_partial_tiles_partial_last_chunk(cornell):
    """20 x 12 (3 x 2 tiles, partial in x and in y), 44 spp (five full chunks and one of 4) as [0, 16) [16, 32) [32, 44), threshold 0.08,
    min_samples 16: tiles stop at 16 and at 32, and the tiles still active receive the partial chunk on the last pass, which their colour
    gets and neither the stop statistic nor the variance does.  After every pass tile_samples, the active count, the three AOVs and the
    variance are the prediction's bits, and a stopped tile's variance stays put; with all AOVs and with colour + variance only."""
    spp, thr, bounds = 44, 0.08, [(0, 16), (16, 32), (32, 44)]
    chunk, g, n_full = chunk_sums(cornell, W, H, spp)
    assert g == 8 and n_full == 5 and chunk.shape[0] == 6
    pred = predict(chunk, W, H, spp, bounds, thr, 16)
    last = pred[-1][0]
    assert last.shape == (2, 3) and (last == 16).any() and (last == 32).any() and (last == spp).any()  # before the GPU is touched
    dev = cornell.device()
    dev.set_adaptive(thr, 16)
    p = cornell.hjr_params(W, H, spp)
    for aovs in (True, False):
        prev = None
        for (b, e), (n_tile, want, active) in zip(bounds, pred):
            what = "%s, adaptive pass [%d, %d)" % ("all AOVs" if aovs else "colour + variance", b, e)
            rc, out, var = render_var(dev, with_range(p, b, e), (H, W, 4), aovs=aovs)
            assert rc == 0, hjr.lib().hjr_last_error()
            assert (dev.tile_samples() == owned_samples(n_tile)).all(), what
            assert dev.adaptive_state()["active_tiles"] == active, what
            assert_same(out, want if aovs else [want[0], None, None], what)
            n_px = np.kron(n_tile, np.ones((8, 8), np.uint32))[:H, :W]
            exp = np.zeros((H, W), f32)
            for n in np.unique(n_px):
                exp = np.where(n_px == n, variance_rule(chunk[:, :, :, 0, :], 8, int(n) // 8, int(n)), exp)
            same_bits(var, exp, what)
            stopped = n_px <= b  # stopped before this pass began
            assert stopped.any() == (b > 0)
            if stopped.any():
                assert np.array_equal(bits(var)[stopped], bits(prev)[stopped]), what + ": a stopped tile's variance moved"
            prev = var
    dev.close()


def test_packed_shard_and_zero_unowned(cornell, dev):
    """Rank 1 of 3 with HJR_FLAG_PACKED: [owned tile][64] floats equal to the same pixels of the single-rank frame (the out-of-image lanes
    of the edge tiles are not compared: the host call copies its whole staging buffer, as for the colour); unpacked with HJR_FLAG_ZERO_UNOWNED: the owned pixels, zeros elsewhere."""
    spp = 40
    rc, full, full_var = render_var(dev, cornell.hjr_params(W, H, spp), (H, W, 4))
    assert rc == 0
    n = hjr.owned_tiles(W, H, 1, 3)
    assert n >= 2
    rc, out, var = render_var(dev, cornell.hjr_params(W, H, spp, rank=1, world_size=3, flags=hjr.FLAG_PACKED), (n, 64, 4))
    assert rc == 0, hjr.lib().hjr_last_error()
    frame = np.zeros((H, W, 4), f32)
    frame[..., 0], frame[..., 1] = full_var, 1
    packed = hjr.pack_tiles(frame, 1, 3)
    inside = packed[..., 1] == 1
    assert inside.any() and (~inside).any()
    assert np.array_equal(bits(var)[inside], bits(packed[..., 0])[inside])
    assert np.array_equal(bits(out[0])[inside], bits(hjr.pack_tiles(full[0], 1, 3))[inside])
    rc, out, var = render_var(dev, cornell.hjr_params(W, H, spp, rank=1, world_size=3, flags=hjr.FLAG_ZERO_UNOWNED), (H, W, 4))
    assert rc == 0, hjr.lib().hjr_last_error()
    own = hjr.owned_tile_mask(W, H, 1, 3)
    same_bits(var, np.where(own, full_var, f32(0)), "ZERO_UNOWNED")


def test_device_pointers(cornell, dev):
    """hjr_render_device_var into torch tensors: the host call's bits; pixels of other ranks' tiles untouched without ZERO_UNOWNED."""
    import torch
    p = cornell.hjr_params(W, H, 40, rank=1, world_size=3)
    color = torch.full((H, W, 4), float(SENTINEL), device="cuda")
    var = torch.full((H, W), float(SENTINEL), device="cuda")
    dev.render_device(p, color.data_ptr(), d_variance=var.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rc, full, full_var = render_var(dev, cornell.hjr_params(W, H, 40), (H, W, 4))
    own = hjr.owned_tile_mask(W, H, 1, 3)
    got = var.cpu().numpy()
    assert np.array_equal(bits(got)[own], bits(full_var)[own]) and (got[~own] == SENTINEL).all()
    assert np.array_equal(bits(color.cpu().numpy())[own], bits(full[0])[own])
