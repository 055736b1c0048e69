"""Adaptive sampling on the GPU (hjr_set_adaptive): converged 8x8 tiles stop between the sample passes of a frame.

The stopping rule is restated here in numpy float32 from the oracle's per-sample values; the GPU must stop the same tiles at the same
passes and write the same AOV bits after every pass, for both kernel families, every integrator and both layouts.  With the setting
off nothing changes; the extremes, shards, state rules, the denoised form and the file level are covered below.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from scene_util import ROOT, Cornell, hjr
from test_gpu_progressive import SENTINEL, assert_same, bits, one_shot, passes, render_raw, with_range

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
ERR_ARG, ERR_STATE = -1, -5
f32 = np.float32
EPS = f32(1e-3)  # HJR_ADAPTIVE_EPS
G = 8            # hjr_sample_granule(spp) for spp <= 512


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


_chunks = {}


def oracle_chunks(cornell, w, h, spp, integ):
    """Chunk sums of the oracle's per-sample values, chunked as test_intermediate_passes_equal_oracle_running_mean chunks them:
    [chunk][y][x][aov][rgb], samples of a chunk added in sample order from +0.0f."""
    key = (w, h, spp, integ)
    if key not in _chunks:
        osc = ob.OracleScene(cornell.arrays, ob.MATH_PORTABLE)
        op = cornell.oracle_params(w, h, spp, integrator=integ)
        chunk = np.zeros((spp // G, h, w, 3, 3), f32)
        for y in range(h):
            for x in range(w):
                for k in range(spp // G):
                    acc = np.zeros((3, 3), f32)
                    for s in range(G * k, G * k + G):
                        acc = acc + np.stack(osc.sample(op, x, y, s))
                    chunk[k, y, x] = acc
        _chunks[key] = chunk
    return _chunks[key]


def tile_of_owned(i, rank, world, tiles_x):
    """(tx, ty) of a rank's i-th owned tile (csrc/hjr_layout.h: hjr_tile_xy)."""
    t = i * world + rank
    ty, c = divmod(t, tiles_x)
    r = ty % tiles_x
    return (c - r if c >= r else c + tiles_x - r), ty


def predict(chunk, w, h, spp, bounds, threshold, min_samples=0):
    """The rule of include/henjou_hip.h in numpy float32.  Returns per pass (n_tile [tiles_y][tiles_x], [color, albedo, normal], tiles
    still active after the pass)."""
    tx_n, ty_n = (w + 7) // 8, (h + 7) // 8
    H, W = ty_n * 8, tx_n * 8
    pad = np.zeros((chunk.shape[0], H, W, 3, 3), f32)
    pad[:, :h, :w] = chunk
    inside = np.zeros((H, W), bool)
    inside[:h, :w] = True
    run = np.zeros((H, W, 3, 3), f32)
    S1 = np.zeros((H, W), f32)
    S2 = np.zeros((H, W), f32)
    stopped = np.zeros((ty_n, tx_n), np.uint32)  # 0 = active, else n_tile
    ms = (min_samples + G - 1) // G * G if min_samples else 2 * G
    idx = np.arange(64)
    res = []
    for b, e in bounds:
        act = np.kron(stopped == 0, np.ones((8, 8), bool))
        for k in range(b // G, (e + G - 1) // G):
            c = pad[k]
            run = np.where(act[..., None, None], run + c, run)
            if k < spp // G:  # the statistic is over full chunks
                y = (c[..., 0, 0] + c[..., 0, 1]) + c[..., 0, 2]
                S1 = np.where(act, S1 + y, S1)
                S2 = np.where(act, S2 + y * y, S2)
        if e < spp and e >= ms and e // G >= 2:
            m, n = f32(e // G), f32(e)
            q = np.maximum(m * S2 - S1 * S1, f32(0))
            err = np.sqrt(q / (m - f32(1))) / (S1 + EPS * n)
            err = np.where(inside, err, f32(0)).astype(f32)
            for j in range(ty_n):
                for i in range(tx_n):
                    if stopped[j, i] == 0:
                        v = err[8 * j:8 * j + 8, 8 * i:8 * i + 8].reshape(64).copy()
                        for kx in (32, 16, 8, 4, 2, 1):
                            v = v + v[idx ^ kx]
                        if v[0] <= f32(threshold) * f32(64):
                            stopped[j, i] = e
        n_tile = np.where(stopped == 0, e, stopped).astype(np.uint32)
        inv = f32(1) / np.kron(n_tile, np.ones((8, 8), np.uint32)).astype(f32)
        img = (run * inv[..., None, None])[:h, :w]
        out = np.ones((3, h, w, 4), f32)
        out[..., :3] = np.moveaxis(img, 2, 0)
        res.append((n_tile, list(out), int((stopped == 0).sum())))
    return res


def owned_samples(n_tile, rank=0, world=1):
    """A predicted n_tile map in the order of hjr_copy_tile_samples."""
    ty_n, tx_n = n_tile.shape
    n = hjr.owned_tiles(tx_n * 8, ty_n * 8, rank, world)
    out = np.zeros(n, np.uint32)
    for i in range(n):
        tx, ty = tile_of_owned(i, rank, world, tx_n)
        out[i] = n_tile[ty, tx]
    return out


def assert_not_vacuous(pred, spp):
    last = pred[-1][0]
    stops = sorted(set(int(v) for v in last.reshape(-1)) - {spp})
    assert len(stops) >= 3, "the prediction stops tiles at %s only" % stops
    assert (last == spp).any(), "the prediction has no tile that never stops"


def even_bounds(spp, step):
    return [(b, b + step) for b in range(0, spp, step)]


def run_adaptive(dev, p, bounds, shape, pred, what):
    """All passes of the frame; after each one the AOV bits and tile_samples equal the prediction."""
    for (b, e), (n_tile, want, active) in zip(bounds, pred):
        rc, out = render_raw(dev, with_range(p, b, e), shape)
        assert rc == 0, hjr.lib().hjr_last_error()
        got_n = dev.tile_samples()
        want_n = owned_samples(n_tile)
        assert (got_n == want_n).all(), "%s pass [%d, %d): tile_samples\n%s\nwant\n%s" % (what, b, e, got_n, want_n)
        assert_same(out, want, "%s pass [%d, %d)" % (what, b, e))
        st = dev.adaptive_state()
        assert st["owned_tiles"] == want_n.size and st["sample_end"] == e
        assert st["active_tiles"] == active
    return out


# (integrator, spp, samples per pass, threshold): the inputs the issue checked on the CPU oracle (48 x 32, min_samples 32)
CASES = {
    "nee": (hjr.INTEGRATOR_NEE, 256, 32, 0.08),
    "mis": (hjr.INTEGRATOR_MIS, 256, 32, 0.08),
    "pt": (hjr.INTEGRATOR_PT, 256, 32, 0.15),
    "nee128": (hjr.INTEGRATOR_NEE, 128, 16, 0.1),
}


@pytest.mark.parametrize("case,layout,pipelines", [("nee", "lds", (1, 2)), ("mis", "lds", (0,)), ("pt", "lds", (0,)), ("nee128", "memory", (1, 2)),
                                                   ("nee128", "lds", (1, 2))])
def test_restatement_tiles_and_aov_bits(cornell, case, layout, pipelines):
    """48 x 32 (24 whole tiles): the numpy restatement of the rule on the oracle's per-sample values predicts, for every pass, which
    tiles have stopped and all three AOVs; the GPU gives the same tile_samples and the same bits.  NEE on both kernel families, MIS,
    Pathtrace; the LDS layout and the forced memory layout (bvh_width 4, lds_bvh 0)."""
    integ, spp, step, thr = CASES[case]
    w, h = 48, 32
    bounds = even_bounds(spp, step)
    pred = predict(oracle_chunks(cornell, w, h, spp, integ), w, h, spp, bounds, thr, 32)
    assert_not_vacuous(pred, spp)  # before the GPU is touched
    dev = cornell.device({"lds": {}, "memory": {"bvh_width": 4, "lds_bvh": 0}}[layout])
    dev.set_adaptive(thr, 32)
    p = cornell.hjr_params(w, h, spp, integrator=integ)
    for pipeline in pipelines:
        dev.set_option("pipeline", pipeline)
        run_adaptive(dev, p, bounds, (h, w, 4), pred, "%s %s pipeline %d" % (case, layout, pipeline))
        assert dev.stats()["lds_mode"] in ((1, 2) if layout == "lds" else (0,))
        n_last = owned_samples(pred[-1][0])
        assert dev.adaptive_state()["samples_rendered"] == 64 * int(n_last.astype(np.uint64).sum())
    # the generator form ends early or at spp and yields the same frames
    dev.set_option("pipeline", 0)
    for (end, c, a, n), (n_tile, want, active) in zip(dev.render_adaptive(p, spp // step), pred):
        assert_same([c, a, n], want, "render_adaptive sample_end %d" % end)


def test_restatement_frame_not_a_multiple_of_8(cornell):
    """44 x 28: edge tiles with out-of-image lanes (e = 0 in the butterfly), same restatement, tile_order 0 (no tile list before the
    filter) and 2 (cost feedback) as well as the default."""
    w, h, spp, step, thr = 44, 28, 128, 16, 0.1
    bounds = even_bounds(spp, step)
    pred = predict(oracle_chunks(cornell, w, h, spp, hjr.INTEGRATOR_NEE), w, h, spp, bounds, thr, 32)
    assert_not_vacuous(pred, spp)
    dev = cornell.device()
    dev.set_adaptive(thr, 32)
    p = cornell.hjr_params(w, h, spp)
    for order in (-1, 0, 2, 2):
        dev.set_option("tile_order", order)
        run_adaptive(dev, p, bounds, (h, w, 4), pred, "44 x 28 tile_order %d" % order)


def test_sized_structs_and_bad_values(cornell):
    """hjr_adaptive / hjr_adaptive_state shorter and longer than the library's follow the sized-struct rule; bad values are HJR_ERR_ARG."""
    L = hjr.lib()
    dev = cornell.device()
    shape = (16, 16, 4)
    p = cornell.hjr_params(16, 16, 64)

    class LongAdaptive(hjr.Adaptive):
        _fields_ = [("future", C.c_uint32 * 4)]

    class ShortAdaptive(hjr._Sized):  # a caller that knows the threshold only: min_samples reads as 0 = two granules
        _fields_ = [("struct_size", C.c_uint32), ("noise_threshold", C.c_float)]

    class LongState(hjr.AdaptiveState):
        _fields_ = [("future", C.c_uint32 * 4)]

    class ShortState(hjr._Sized):
        _fields_ = [("struct_size", C.c_uint32), ("owned_tiles", C.c_uint32), ("active_tiles", C.c_uint32)]

    la = LongAdaptive()
    la.noise_threshold, la.min_samples = 1e30, 32
    for i in range(4):
        la.future[i] = 0xABABABAB
    assert L.hjr_set_adaptive(dev._h, C.byref(la)) == 0
    passes(dev, p, [(0, 16), (16, 32)], shape)
    assert list(dev.tile_samples()) == [32] * 4
    sa = ShortAdaptive()
    sa.noise_threshold = 1e30
    assert L.hjr_set_adaptive(dev._h, C.byref(sa)) == 0
    passes(dev, p, [(0, 8), (8, 16), (16, 24)], shape)
    assert list(dev.tile_samples()) == [16] * 4  # min_samples 0: two granules
    ls = LongState()
    for i in range(4):
        ls.future[i] = 0xCDCDCDCD
    assert L.hjr_get_adaptive_state(dev._h, C.byref(ls)) == 0
    assert (ls.owned_tiles, ls.active_tiles, ls.sample_end, ls.samples_rendered) == (4, 0, 24, 4 * 64 * 16)
    assert ls.struct_size == C.sizeof(ls) and list(ls.future) == [0xCDCDCDCD] * 4
    buf = (C.c_ubyte * 64)(*([0xEE] * 64))
    ss = ShortState.from_buffer(buf)
    ss.struct_size = C.sizeof(ShortState)
    assert L.hjr_get_adaptive_state(dev._h, C.byref(ss)) == 0
    assert (ss.owned_tiles, ss.active_tiles) == (4, 0) and all(v == 0xEE for v in bytes(buf)[C.sizeof(ShortState):])
    zero = hjr.Adaptive()
    zero.struct_size = 0
    assert L.hjr_set_adaptive(dev._h, C.byref(zero)) == ERR_ARG
    zs = hjr.AdaptiveState()
    zs.struct_size = 0
    assert L.hjr_get_adaptive_state(dev._h, C.byref(zs)) == ERR_ARG
    for bad in (-0.5, float("inf"), float("-inf"), float("nan")):
        a = hjr.Adaptive()
        a.noise_threshold = bad
        assert L.hjr_set_adaptive(dev._h, C.byref(a)) == ERR_ARG, bad
        assert b"noise_threshold" in L.hjr_last_error()
    n = np.zeros(8, np.uint32)
    dev.set_adaptive(1e30)
    passes(dev, p, [(0, 16)], shape)
    assert L.hjr_copy_tile_samples(dev._h, n.ctypes.data, 3) == ERR_ARG
    assert L.hjr_copy_tile_samples(dev._h, None, 4) == ERR_ARG
    assert L.hjr_set_adaptive(dev._h, None) == 0  # NULL: off
    with pytest.raises(hjr.HjrError):
        dev.adaptive_state()


def test_off_is_off(cornell):
    """Without hjr_set_adaptive, and after hjr_set_adaptive with threshold 0, the passes end in the one-shot frame as they always did
    and no adaptive state exists."""
    shape = (24, 32, 4)
    p = cornell.hjr_params(32, 24, 64)
    bounds = [(0, 16), (16, 40), (40, 64)]
    dev = cornell.device()
    ref = one_shot(dev, p, shape)
    plain = passes(dev, p, bounds, shape)
    assert_same(plain[-1], ref, "passes, never adaptive")
    with pytest.raises(hjr.HjrError, match="adaptive"):
        dev.adaptive_state()
    with pytest.raises(hjr.HjrError, match="adaptive"):
        dev.tile_samples()
    dev.set_adaptive(0.5)
    dev.set_adaptive(0.0)
    off = passes(dev, p, bounds, shape)
    for a, b, (s, e) in zip(off, plain, bounds):
        assert_same(a, b, "threshold 0, pass [%d, %d)" % (s, e))
    with pytest.raises(hjr.HjrError, match="adaptive"):
        dev.adaptive_state()


@pytest.mark.parametrize("min_samples,first", [(0, 16), (96, 96), (20, 24)])
def test_extremes_everything_stops_at_the_first_boundary(cornell, min_samples, first):
    """noise_threshold 1e30: every tile stops at the first boundary at or after max(min_samples, two granules); the frame is the
    non-adaptive running mean at that boundary, and a later pass (counting launch) renders 0 samples and rewrites the same bits."""
    w, h, spp = 40, 24, 128
    shape = (h, w, 4)
    p = cornell.hjr_params(w, h, spp)
    bounds = [(8 * k, 8 * k + 8) for k in range(spp // 8)]
    dev = cornell.device()
    upto = [b for b in bounds if b[1] <= first]
    plain = passes(dev, p, upto, shape)[-1]
    dev.set_adaptive(1e30, min_samples)
    got = passes(dev, p, upto, shape)
    assert_same(got[-1], plain, "adaptive frame at the stop boundary")
    st = dev.adaptive_state()
    assert st == {"owned_tiles": 15, "active_tiles": 0, "sample_end": first, "samples_rendered": 15 * 64 * first}
    assert (dev.tile_samples() == first).all()
    if len(upto) > 1:  # one boundary earlier nothing had stopped
        dev.set_adaptive(1e30, min_samples)
        passes(dev, p, upto[:-1], shape)
        assert dev.adaptive_state()["active_tiles"] == 15
        passes(dev, p, upto[-1:], shape)
    q = with_range(p, first, first + 8)
    q.flags |= hjr.FLAG_STATS
    rc, later = render_raw(dev, q, shape)  # fresh sentinel-filled buffers
    assert rc == 0, hjr.lib().hjr_last_error()
    assert dev.stats()["samples"] == 0
    assert_same(later, plain, "a pass with no active tile")
    assert dev.adaptive_state() == {"owned_tiles": 15, "active_tiles": 0, "sample_end": first + 8, "samples_rendered": 15 * 64 * first}
    assert (dev.tile_samples() == first).all()


def test_tiny_threshold_stops_only_what_the_rule_says(cornell):
    """noise_threshold 1e-30 (the cost-of-the-machinery configuration): the restatement decides which tiles stop (those whose q comes
    out as exactly 0); every tile that never stops ends with the one-shot frame's bits."""
    w, h, spp, step = 48, 32, 128, 16
    shape = (h, w, 4)
    bounds = even_bounds(spp, step)
    pred = predict(oracle_chunks(cornell, w, h, spp, hjr.INTEGRATOR_NEE), w, h, spp, bounds, 1e-30, 0)
    assert (pred[-1][0] == spp).any()
    p = cornell.hjr_params(w, h, spp)
    dev = cornell.device()
    ref = one_shot(dev, p, shape)
    dev.set_adaptive(1e-30)
    got = run_adaptive(dev, p, bounds, shape, pred, "threshold 1e-30")
    n = dev.tile_samples()
    for i in range(n.size):
        tx, ty = tile_of_owned(i, 0, 1, 6)
        if n[i] == spp:
            sl = (slice(8 * ty, 8 * ty + 8), slice(8 * tx, 8 * tx + 8))
            assert_same([a[sl] for a in got], [a[sl] for a in ref], "tile %d never stopped" % i)


def test_shards_adapt_on_their_own(cornell):
    """Ranks 0, 1, 2 of 3 with HJR_FLAG_PACKED, each adaptive on its own tiles, unpacked into one frame: bit-equal to the one-rank
    adaptive frame after every pass, and the interleaved tile_samples agree."""
    w, h, spp, step, thr = 48, 32, 128, 16, 0.1
    bounds = even_bounds(spp, step)
    dev = cornell.device()
    dev.set_adaptive(thr, 32)
    whole, whole_n = [], []
    for b, e in bounds:
        rc, out = render_raw(dev, with_range(cornell.hjr_params(w, h, spp), b, e), (h, w, 4))
        assert rc == 0
        whole.append(out)
        whole_n.append(dev.tile_samples())
    assert len(set(whole_n[-1].tolist())) >= 3
    frames = [[np.zeros((h, w, 4), f32) for _ in range(3)] for _ in bounds]
    tiles = [np.zeros(24, np.uint32) for _ in bounds]
    for rank in range(3):
        n = hjr.owned_tiles(w, h, rank, 3)
        p = cornell.hjr_params(w, h, spp, rank=rank, world_size=3, flags=hjr.FLAG_PACKED)
        for k, (b, e) in enumerate(bounds):
            rc, out = render_raw(dev, with_range(p, b, e), (n, 64, 4))
            assert rc == 0, hjr.lib().hjr_last_error()
            for a in range(3):
                hjr.unpack_tiles(out[a], frames[k][a], rank, 3)
            tiles[k][rank::3] = dev.tile_samples()
    for k, (b, e) in enumerate(bounds):
        assert_same(frames[k], whole[k], "3 ranks, pass [%d, %d)" % (b, e))
        assert (tiles[k] == whole_n[k]).all()


def test_state_rules(cornell):
    """hjr_set_adaptive between two passes: the continuing pass is HJR_ERR_STATE and leaves its outputs untouched; a whole-frame render
    while adaptive is set is the plain one-shot frame and leaves no adaptive state."""
    shape = (24, 32, 4)
    p = cornell.hjr_params(32, 24, 64)
    dev = cornell.device()
    ref = one_shot(dev, p, shape)
    for first, then in ((None, 0.1), (0.1, 0.2), (0.1, 0.0)):
        dev.set_adaptive(first or 0.0)
        passes(dev, p, [(0, 16)], shape)
        dev.set_adaptive(then)
        rc, out = render_raw(dev, with_range(p, 16, 32), shape)
        assert rc == ERR_STATE, (rc, hjr.lib().hjr_last_error())
        assert "no progressive frame" in hjr.lib().hjr_last_error().decode()
        for a in out:
            assert (bits(a) == bits(np.full(shape, SENTINEL, f32))).all(), "a refused pass wrote its output"
    dev.set_adaptive(1e30)
    assert_same(one_shot(dev, p, shape), ref, "whole-frame render with adaptive set (sample_end 0)")
    assert_same(one_shot(dev, with_range(p, 0, 64), shape), ref, "whole-frame render with adaptive set ([0, spp))")
    with pytest.raises(hjr.HjrError, match="adaptive"):
        dev.adaptive_state()
    passes(dev, p, [(0, 16)], shape)
    assert dev.adaptive_state()["active_tiles"] == 0
    one_shot(dev, p, shape)  # ends the progressive frame and its adaptive state
    with pytest.raises(hjr.HjrError, match="adaptive"):
        dev.adaptive_state()


@pytest.mark.parametrize("mode", [hjr.MODE_DENOISE, hjr.MODE_DENOISE_UPSCALE2X])
def test_denoised_adaptive_passes(cornell, mode):
    """hjr_render_denoised over adaptive passes filters the adaptive frame: equal to hjr_denoise of the AOVs the same passes give."""
    w, h, spp, step, thr = 48, 32, 128, 16, 0.1
    bounds = even_bounds(spp, step)
    p = cornell.hjr_params(w, h, spp)
    dev = cornell.device()
    dev.set_adaptive(thr, 32)
    last = passes(dev, p, bounds, (h, w, 4))[-1]
    n = dev.tile_samples()
    assert len(set(n.tolist())) >= 3
    want = dev.denoise(mode, *last)
    dev.set_adaptive(thr, 32)
    outs = [dev.render_denoised(with_range(p, b, e), mode) for b, e in bounds]
    assert (bits(outs[-1]) == bits(want)).all()
    assert (dev.tile_samples() == n).all()


def test_file_level_adaptive_png(tmp_path, cornell):
    """henjou_cli with "noise_threshold" / "min_samples" writes the PNG float4_to_srgb8 of the Python adaptive frame gives: as a single
    process (hjr_render_file) and as a --rank world of one; the frame stops early and says so."""
    assert os.path.exists(CLI), "henjou_cli is not built"
    w, h, spp, thr = 48, 32, 128, 0.15
    work = tmp_path / "run"
    shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
    shutil.copytree(os.path.join(hjr.ASSETS, "LUT"), work / "LUT")
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Image"].update(image_width=w, image_height=h, max_spp=spp)
    ro["Henjou_HIP"] = {"noise_threshold": thr, "min_samples": 32}  # no "passes": 8 passes of 16
    dev = cornell.device()
    dev.set_adaptive(thr, 32)
    frames = list(dev.render_adaptive(cornell.hjr_params(w, h, spp), 8, want_aovs=False))
    n = dev.tile_samples()
    assert len(frames) < 8 and dev.adaptive_state()["active_tiles"] == 0 and len(set(n.tolist())) >= 2
    want = hjr.float4_to_srgb8(frames[-1][1])[::-1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for name, args in (("single", []), ("rank", ["--rank", "0", "--world", "1"])):
        ro["Image"]["image_name"] = name
        (work / "render_option.json").write_text(json.dumps(ro))
        q = subprocess.run([CLI, "render_option.json"] + args, cwd=work, capture_output=True, text=True, timeout=300, env=env)
        assert q.returncode == 0, q.stdout + q.stderr
        assert "0 of %d tiles active at %d spp" % (n.size, frames[-1][0]) in q.stderr, q.stderr
        got = hjr.load_png(str(work / (name + "_001.png")))
        assert np.array_equal(got, want), "%s: %d pixels differ" % (name, int(np.sum(np.any(got != want, axis=-1))))
