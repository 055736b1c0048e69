"""Render windows on the GPU (hjr_params_window.window, DESIGN.md §4 rule 12): a window launch writes the crop of the whole-frame launch.

A pixel's value depends on its full-frame coordinates, the sample number, the seed and spp only, so every AOV of a window must equal
full[y0:y1, x0:x1] bit for bit: both kernel families, every integrator, shards, sample passes, adaptive sampling and the firefly rules.
Nothing a context keeps between launches may leak from one window into the next.  Shapes: 43 x 29 is 6 x 4 tiles with ragged right and
top edges; 16 spp is two chunks, 8 spp one, 32 spp four (the variance AOV needs two full chunks).
"""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
from scene_util import Cornell, hjr
from test_gpu_adaptive import oracle_chunks, predict
from test_gpu_progressive import SENTINEL, bits

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -5
W, H = 43, 29
WINDOWS = [(8, 8, 32, 24),    # interior, tile-sized extent
           (0, 0, 8, 8),      # one tile
           (8, 16, 21, 27),   # ragged ends inside the frame
           (16, 8, 43, 29),   # reaches both ragged frame edges
           (0, 0, 43, 29)]    # the frame as a window
INTEGRATORS = (hjr.INTEGRATOR_NEE, hjr.INTEGRATOR_PT, hjr.INTEGRATOR_MIS)


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


def with_window(p, win, begin=None, end=None, **kw):
    q = hjr.ParamsV3()
    C.memmove(C.addressof(q), C.addressof(p), min(C.sizeof(p), C.sizeof(q)))
    q.struct_size = C.sizeof(q)
    q.window = (C.c_uint32 * 4)(*(win or (0, 0, 0, 0)))
    if begin is not None:
        q.sample_begin, q.sample_end = begin, end
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def win_shape(win, w=W, h=H):
    return (win[3] - win[1], win[2] - win[0]) if win else (h, w)


def render_raw(dev, p, shape, aovs=True, var=False):
    """hjr_render_var into sentinel-filled host arrays of exactly `shape` (+ one guard row behind each, which must stay sentinel):
    (status, [color, albedo, normal, variance])."""
    guard = shape[1] if len(shape) > 1 else 64
    bufs = []
    for i in range(4):
        want = i == 0 or (i < 3 and aovs) or (i == 3 and var)
        n = int(np.prod(shape)) * (4 if i < 3 else 1)
        bufs.append(np.full(n + guard * 4, SENTINEL, np.float32) if want else None)
    rc = hjr.lib().hjr_render_var(dev._h, C.byref(p), *[None if b is None else b.ctypes.data for b in bufs])
    out = []
    for i, b in enumerate(bufs):
        if b is None:
            out.append(None)
            continue
        n = int(np.prod(shape)) * (4 if i < 3 else 1)
        assert (b[n:] == SENTINEL).all(), "AOV %d: written behind the window's last pixel" % i
        out.append(b[:n].reshape(tuple(shape) + ((4,) if i < 3 else ())))
    return rc, out


def ok(dev, p, shape, aovs=True, var=False):
    rc, out = render_raw(dev, p, shape, aovs, var)
    assert rc == 0, hjr.lib().hjr_last_error()
    for a in out:
        assert a is None or not (a == SENTINEL).any(), "an output pixel was not written"
    return out


def crop(a, win):
    return None if a is None else a[win[1]:win[3], win[0]:win[2]]


def assert_crop(got, full, win, what):
    for name, g, f in zip(("color", "albedo", "normal", "variance"), got, full):
        if f is None:
            assert g is None, what
            continue
        want = crop(f, win)
        assert g.shape == want.shape, "%s, %s: shape %s, want %s" % (what, name, g.shape, want.shape)
        same = bits(g) == bits(want)
        assert same.all(), "%s, %s: %d of %d values differ from the crop" % (what, name, int((~same).sum()), same.size)


@pytest.mark.parametrize("pipeline", [1, 2])
def test_window_is_the_crop(cornell, pipeline):
    """1. Colour, albedo, normal (8 and 16 spp) and with them the variance AOV (32 spp) of the five windows equal the crop of the whole
    frame: megakernel (pipeline 1) and wavefront (2) family, NEE / Pathtrace / MIS, sentinel-filled outputs of exactly the window's size."""
    dev = cornell.device({"pipeline": pipeline})
    for integ in INTEGRATORS:
        for spp in (8, 16, 32):
            p = cornell.hjr_params(W, H, spp, integrator=integ)
            full = ok(dev, p, (H, W), var=spp == 32)
            assert dev.stats()["pipeline"] == pipeline - 1
            for win in WINDOWS:
                got = ok(dev, with_window(p, win), win_shape(win), var=spp == 32)
                assert_crop(got, full, win, "pipeline %d integrator %d %d spp window %s" % (pipeline, integ, spp, win))
            if spp == 32:
                assert (full[3] != hjr.VARIANCE_UNKNOWN).any()


def test_window_equals_oracle_rect(cornell):
    """2. Window (8, 16, 21, 27), NEE, 16 spp equals the oracle rendered in that rectangle, and a counting launch has the oracle's samples,
    closest_rays and shadow_rays for the rectangle."""
    win = (8, 16, 21, 27)
    osc = ob.OracleScene(cornell.arrays, ob.MATH_PORTABLE)
    oc, oa, on, ost = osc.render(cornell.oracle_params(W, H, 16, rect=win))
    dev = cornell.device()
    p = cornell.hjr_params(W, H, 16)
    got = ok(dev, with_window(p, win), win_shape(win))
    assert_crop(got, (oc, oa, on), win, "oracle rect")
    got = ok(dev, with_window(p, win, flags=hjr.FLAG_STATS), win_shape(win))
    assert_crop(got, (oc, oa, on), win, "oracle rect, counting launch")
    st = dev.stats()
    assert ost["samples"] == (win[2] - win[0]) * (win[3] - win[1]) * 16
    for k in ("samples", "closest_rays", "shadow_rays"):
        assert st[k] == ost[k], "%s: %d, oracle %d" % (k, st[k], ost[k])


@pytest.mark.parametrize("world", [2, 3])
def test_window_shards(cornell, world):
    """3. Shards of a window are shards of the window's tiles: the ranks' packed outputs, unpacked at the window's size, and the sum of
    their ZERO_UNOWNED outputs both give the crop."""
    dev = cornell.device()
    p = cornell.hjr_params(W, H, 16)
    full = ok(dev, p, (H, W))
    for win in (WINDOWS[2], WINDOWS[3]):
        wh, ww = win_shape(win)
        frames = [np.full((wh, ww, 4), SENTINEL, np.float32) for _ in range(3)]
        sums = [np.zeros((wh, ww, 4), np.float32) for _ in range(3)]
        for rank in range(world):
            n = hjr.owned_tiles(ww, wh, rank, world)
            assert n > 0
            q = with_window(p, win, rank=rank, world_size=world, flags=hjr.FLAG_PACKED)
            packed = ok(dev, q, (n, 64))[:3]
            for f, pk in zip(frames, packed):
                hjr.unpack_tiles(pk, f, rank, world)
            q = with_window(p, win, rank=rank, world_size=world, flags=hjr.FLAG_ZERO_UNOWNED)
            rc, part = render_raw(dev, q, (wh, ww))
            assert rc == 0, hjr.lib().hjr_last_error()
            mask = hjr.owned_tile_mask(ww, wh, rank, world)
            for s, a in zip(sums, part[:3]):
                assert (a[~mask] == 0).all() and not (a[mask] == SENTINEL).any()
                s += a
        assert_crop(frames, full, win, "world %d packed window %s" % (world, win))
        assert_crop(sums, full, win, "world %d zero-unowned window %s" % (world, win))


def test_window_passes_and_state(cornell):
    """4. 32 spp in the passes of pass_bounds(32, 4): the last pass equals the one-shot window; a continuing pass with another window, or
    with none, is HJR_ERR_STATE, leaves its outputs untouched, and the corrected pass then finishes the frame."""
    dev = cornell.device()
    p = cornell.hjr_params(W, H, 32)
    bounds = hjr.pass_bounds(32, 4)
    assert len(bounds) == 4
    full = ok(dev, p, (H, W), var=True)
    for win in (WINDOWS[2], WINDOWS[3]):
        shape = win_shape(win)
        one = ok(dev, with_window(p, win), shape, var=True)
        assert_crop(one, full, win, "one-shot window %s" % (win,))
        for k, (b, e) in enumerate(bounds):
            if k == 2:  # a pass that does not repeat the window
                for other in (WINDOWS[0], None):
                    rc, out = render_raw(dev, with_window(p, other, b, e), win_shape(other), var=True)
                    assert rc == ERR_STATE and b"window" in hjr.lib().hjr_last_error()
                    assert all((a == SENTINEL).all() for a in out)
            got = ok(dev, with_window(p, win, b, e), shape, var=True)
        assert_crop(got, full, win, "last pass, window %s" % (win,))


def test_window_adaptive(cornell):
    """5. Frame 48 x 32, 64 spp in 8 passes, threshold 0.1 (test_gpu_adaptive's): after every pass the window (8, 8, 40, 24) holds the crop
    of the whole frame's adaptive run and its tile_samples are those of the frame's tiles under it.  The restatement of the stop rule on the
    oracle's samples shows tiles of both kinds inside the window."""
    w, h, spp, thr, win = 48, 32, 64, 0.1, (8, 8, 40, 24)
    bounds = [(b, b + 8) for b in range(0, spp, 8)]
    pred = predict(oracle_chunks(cornell, w, h, spp, hjr.INTEGRATOR_NEE), w, h, spp, bounds, thr)
    n_last = pred[-1][0][win[1] // 8:win[3] // 8, win[0] // 8:win[2] // 8]
    assert (n_last < spp).any() and (n_last == spp).any(), "the window needs tiles that stop and tiles that do not:\n%s" % n_last
    dev_f, dev_w = cornell.device(), cornell.device()
    dev_f.set_adaptive(thr)
    dev_w.set_adaptive(thr)
    p = cornell.hjr_params(w, h, spp)
    tiles_x = w // 8
    wtx, wty = (win[2] - win[0]) // 8, (win[3] - win[1]) // 8
    for b, e in bounds:
        full = ok(dev_f, with_window(p, None, b, e), (h, w), var=True)
        n_full = np.zeros((h // 8, tiles_x), np.uint32)
        for i, n in enumerate(dev_f.tile_samples()):
            ty, c = divmod(i, tiles_x)
            n_full[ty, (c - ty % tiles_x) % tiles_x] = n
        got = ok(dev_w, with_window(p, win, b, e), win_shape(win), var=True)
        assert_crop(got, full, win, "adaptive pass [%d, %d)" % (b, e))
        n_win = np.zeros((wty, wtx), np.uint32)
        for i, n in enumerate(dev_w.tile_samples()):
            ty, c = divmod(i, wtx)
            n_win[ty, (c - ty % wtx) % wtx] = n
        assert (n_win == n_full[win[1] // 8:win[3] // 8, win[0] // 8:win[2] // 8]).all(), "pass [%d, %d)\n%s" % (b, e, n_win)
        assert dev_w.adaptive_state()["owned_tiles"] == wtx * wty
    assert (n_win == n_last).all()


def test_window_firefly(cornell):
    """6. 64 x 40, 64 spp, firefly_clamp 4: window (16, 8, 48, 32) equals the crop of the clamped frame, one-shot and with
    firefly_clamp_passes in 4 passes; the rule acted inside the window."""
    w, h, spp, win = 64, 40, 64, (16, 8, 48, 32)
    dev = cornell.device()
    p = cornell.hjr_params(w, h, spp)
    plain = ok(dev, p, (h, w))
    dev.set_option("firefly_clamp", 4)
    full = ok(dev, p, (h, w), var=True)
    assert (bits(crop(full[0], win)) != bits(crop(plain[0], win))).any(), "no pixel of the window is clamped"
    got = ok(dev, with_window(p, win), win_shape(win), var=True)
    assert_crop(got, full, win, "firefly_clamp one-shot")
    assert dev.stats()["firefly_clamped"] > 0
    dev.set_option("firefly_clamp_passes", 1)
    for b, e in hjr.pass_bounds(spp, 4):
        full_p = ok(dev, with_window(p, None, b, e), (h, w), var=True)
    assert_crop(full_p, full, (0, 0, w, h), "whole frame in passes")
    for b, e in hjr.pass_bounds(spp, 4):
        got = ok(dev, with_window(p, win, b, e), win_shape(win), var=True)
    assert_crop(got, full, win, "firefly_clamp_passes, last pass")


def test_window_state_hygiene(cornell):
    """7. One context renders the whole frame, window A, window B of another size and the whole frame again, under the measured-cost tile
    order (tile_order 2) and as unfinished progressive frames in between: every result equals a fresh context's."""
    p = cornell.hjr_params(W, H, 16)
    seq = [None, WINDOWS[0], WINDOWS[3], WINDOWS[2], None, WINDOWS[2], None]
    fresh = []
    for win in seq[:4]:
        fresh.append(ok(cornell.device(), with_window(p, win), win_shape(win), var=True))
    want = {None: fresh[0], WINDOWS[0]: fresh[1], WINDOWS[3]: fresh[2], WINDOWS[2]: fresh[3]}
    dev = cornell.device({"tile_order": 2})
    for k, win in enumerate(seq):
        ok(dev, with_window(p, win, 0, 8), win_shape(win))  # an unfinished progressive frame of this rectangle is left behind
        got = ok(dev, with_window(p, win), win_shape(win), var=True)
        assert_crop(got, want[win], (0, 0) + win_shape(win)[::-1], "step %d, window %s" % (k, win))


def test_window_refusals(cornell):
    """8. A bad window, and a window at an entry point that takes whole frames only, is HJR_ERR_ARG with a text naming the field and leaves
    the outputs untouched; a caller with the shorter ParamsV2 still gets the whole frame."""
    L = hjr.lib()
    dev = cornell.device()
    p = cornell.hjr_params(W, H, 16)
    full = ok(dev, p, (H, W))
    for bad in ((4, 8, 32, 24), (8, 8, 44, 24), (8, 8, 32, 30), (16, 8, 16, 24), (24, 8, 16, 24), (8, 12, 32, 24), (8, 24, 32, 24)):
        shape = (max(bad[3] - bad[1], 1), max(bad[2] - bad[0], 1))
        rc, out = render_raw(dev, with_window(p, bad), shape)
        assert rc == ERR_ARG and b"window" in L.hjr_last_error(), bad
        assert all((a == SENTINEL).all() for a in out if a is not None), bad
    q = with_window(p, WINDOWS[0])
    out = np.full((H, W, 4), SENTINEL, np.float32)
    assert L.hjr_render_denoised(dev._h, C.byref(q), hjr.MODE_DENOISE, out.ctypes.data, W, H) == ERR_ARG and b"window" in L.hjr_last_error()
    assert (out == SENTINEL).all()
    gb = np.full((H, W, 12), SENTINEL, np.float32)
    assert L.hjr_render_gbuffer(dev._h, C.byref(q), gb.ctypes.data) == ERR_ARG and b"window" in L.hjr_last_error()
    assert (gb == SENTINEL).all()
    dev_t = cornell.device({"denoise_temporal": 1, "adaptive_temporal": 1})
    rc, out = render_raw(dev_t, q, win_shape(WINDOWS[0]))
    assert rc == ERR_ARG and b"adaptive_temporal" in L.hjr_last_error() and all((a == SENTINEL).all() for a in out if a is not None)
    short = hjr.ParamsV2.from_buffer_copy(q)  # a caller whose struct ends before the window: struct_size says so
    short.struct_size = C.sizeof(hjr.ParamsV2)
    assert short.struct_size < q.struct_size
    rc, out = render_raw(dev, short, (H, W))
    assert rc == 0
    assert_crop(out, full, (0, 0, W, H), "ParamsV2 caller")


def test_blit_window_device(cornell):
    """9. hjr_blit_window_device of the five windows' colour into a sentinel frame on the device reproduces the whole frame where a window
    covers it and leaves the sentinel elsewhere; a window outside the frame is HJR_ERR_ARG."""
    import torch
    dev = cornell.device()
    p = cornell.hjr_params(W, H, 16)
    full = ok(dev, p, (H, W))[0]
    for wins in ([w] for w in WINDOWS[:4]):
        frame = torch.full((H, W, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
        covered = np.zeros((H, W), bool)
        for win in wins:
            img = torch.from_numpy(ok(dev, with_window(p, win), win_shape(win))[0].copy()).cuda()
            dev.blit_window_device(img.data_ptr(), win, frame.data_ptr(), W, H)
            covered[win[1]:win[3], win[0]:win[2]] = True
        dev.synchronize()
        got = frame.cpu().numpy()
        assert (bits(got[covered]) == bits(full[covered])).all(), wins
        assert (got[~covered] == SENTINEL).all(), wins
    frame = torch.full((H, W, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    for win in WINDOWS:  # all five, overlapping: the whole frame
        img = torch.from_numpy(ok(dev, with_window(p, win), win_shape(win))[0].copy()).cuda()
        dev.blit_window_device(img.data_ptr(), win, frame.data_ptr(), W, H)
    dev.synchronize()
    assert (bits(frame.cpu().numpy()) == bits(full)).all()
    with pytest.raises(hjr.HjrError, match="window"):
        dev.blit_window_device(frame.data_ptr(), (8, 8, 44, 24), frame.data_ptr(), W, H)
