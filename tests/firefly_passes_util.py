"""The firefly clamp on sample passes and adaptive frames (option "firefly_clamp_passes"; include/henjou_hip.h "Firefly clamp on sample
passes", DESIGN.md §4 rule 10) restated in numpy float32 on the oracle's chunk sums.  No GPU needed; tools may import it.

Built on firefly_util.firefly_rule (rule 9, which rule 10 applies to the chunks a pixel has received) and on the butterfly of
tests/test_gpu_adaptive.py::predict (rule 6).  Every operation is one IEEE fp32 operation in the order the header writes it, so the
result equals the device's bit for bit.  `stat="raw"` keeps rule 6's own statistic for the stop decision while the colour is clamped: what
the vacuity checks and the rehearsal table compare the rule against."""
import ctypes as C

import numpy as np

from denoise_var_util import variance_rule
from firefly_util import EPS as FIREFLY_EPS
from firefly_util import f32, firefly_rule, granule_of, lower_median

ADAPTIVE_EPS = f32(1e-3)  # HJR_ADAPTIVE_EPS


def chunks_received(g, spp, n):
    """Chunk sums a pixel has received after n samples: the m_n = n // g full ones and, when n = spp is no multiple of g, the partial one."""
    assert n <= spp and (n % g == 0 or n == spp)
    return n // g + (1 if n % g else 0)


def pass_rule(color_chunk, g, spp, n, kappa):
    """Step 2 of rule 10: the colour a pass that ends at n writes, from the colour chunk sums [n_chunks, ..., 3] of the frame.  Rule 9 over
    the received chunks with m_n, r_n, n in place of m, r, spp; the plain running mean when m_n < 4.  Returns firefly_rule's triple."""
    return firefly_rule(color_chunk[:chunks_received(g, spp, n)], g, n, kappa)


def clamped_statistic(color_chunk, g, m, kappa):
    """Step 4 of rule 10: (S1', S2') over the m >= 4 full chunks [0, m) of every pixel, y'_k = (c.x s_k + c.y s_k) + c.z s_k with the pass's
    limit, in chunk order from +0.0f."""
    c = np.ascontiguousarray(color_chunk[:m], f32)
    y = (c[..., 0] + c[..., 1]) + c[..., 2]
    lim = f32(kappa) * lower_median(y) + FIREFLY_EPS * f32(g)
    S1 = np.zeros(y.shape[1:], f32)
    S2 = np.zeros(y.shape[1:], f32)
    for k in range(m):
        over = y[k] > lim
        s = np.ones_like(lim)
        np.divide(lim, y[k], out=s, where=over)
        yc = (c[k, ..., 0] * s + c[k, ..., 1] * s) + c[k, ..., 2] * s
        S1 = S1 + yc
        S2 = S2 + yc * yc
    return S1, S2


def predict(chunk, g, w, h, spp, bounds, kappa, threshold=0.0, min_samples=0, stat="clamped"):
    """Rule 10 for a frame rendered in the passes `bounds`; threshold 0: a plain progressive frame (no stop decisions).
    chunk: float32 [n_chunks][h][w][A][3], A = 1 (colour) or 3 (colour, albedo, normal) chunk sums of the whole frame, the partial chunk last.
    stat: "clamped" (the rule) or "raw" (rule 6's statistic whatever m_n; the colour is clamped all the same).  kappa 0: rules 5 / 6 alone.
    Returns per pass a dict: n_tile uint32 [tiles_y][tiles_x] (samples each tile's mean is over), aovs (A frames [h][w][4]), variance
    float32 [h][w] (rule 7, raw), active (tiles still active after the pass), count (scaled (pixel, chunk) pairs in the written colour)."""
    chunk = np.ascontiguousarray(chunk, f32)
    A = chunk.shape[3]
    col = chunk[:, :, :, 0, :]
    n_full = spp // g
    assert chunk.shape[0] == chunks_received(g, spp, spp)
    tx_n, ty_n = (w + 7) // 8, (h + 7) // 8
    H, W = ty_n * 8, tx_n * 8
    pad = np.zeros((chunk.shape[0], H, W, 3), f32)  # the butterfly runs over whole tiles: out-of-image lanes carry e = 0
    pad[:, :h, :w] = col
    inside = np.zeros((H, W), bool)
    inside[:h, :w] = True
    run = np.zeros((h, w, A, 3), f32)
    S1 = np.zeros((H, W), f32)
    S2 = np.zeros((H, W), f32)
    stopped = np.zeros((ty_n, tx_n), np.uint32)  # 0 = active, else n_tile
    ms = (min_samples + g - 1) // g * g if min_samples else 2 * g
    idx = np.arange(64)
    res = []
    for b, e in bounds:
        act = np.kron(stopped == 0, np.ones((8, 8), bool))
        for k in range(b // g, (e + g - 1) // g):
            run = np.where(act[:h, :w, None, None], run + chunk[k], run)
            if k < n_full:  # the raw statistic is over full chunks
                y = (pad[k][..., 0] + pad[k][..., 1]) + pad[k][..., 2]
                S1 = np.where(act, S1 + y, S1)
                S2 = np.where(act, S2 + y * y, S2)
        if threshold > 0 and e < spp and e >= ms and e // g >= 2:
            m, n = e // g, f32(e)
            D1, D2 = (S1, S2) if (stat == "raw" or kappa <= 0 or m < 4) else clamped_statistic(pad, g, m, kappa)
            q = np.maximum(f32(m) * D2 - D1 * D1, f32(0))
            err = np.sqrt(q / (f32(m) - f32(1))) / (D1 + ADAPTIVE_EPS * n)
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
        n_px = np.kron(n_tile, np.ones((8, 8), np.uint32))[:h, :w]
        img = run * (f32(1) / n_px.astype(f32))[..., None, None]
        var = np.zeros((h, w), f32)
        count = 0
        for nv in sorted(set(int(v) for v in n_tile.reshape(-1))):  # a stopped tile: the rule over its own chunks, n = n_tile
            sel = n_px == nv
            var[sel] = variance_rule(col[:, sel], g, nv // g, nv)
            if kappa > 0:
                rgb, cnt, _ = pass_rule(col[:, sel], g, spp, nv, kappa)
                img[sel, 0] = rgb
                count += cnt
        out = np.ones((A, h, w, 4), f32)
        out[..., :3] = np.moveaxis(img, 2, 0)
        res.append({"n_tile": n_tile, "aovs": list(out), "variance": var, "active": int((stopped == 0).sum()), "count": count})
    return res


def samples_share(n_tile, spp):
    """Share of the frame's samples an adaptive frame rendered (whole tiles, as the library counts them)."""
    return float(n_tile.astype(np.float64).sum() / (n_tile.size * spp))


_chunks = {}


def oracle_aov_chunks(cornell, w, h, spp, integrator=0, camera=None, seed=1):
    """firefly_util.oracle_color_chunks with the albedo and normal sums next to the colour's: [n_chunks][h][w][3 AOVs][3] float32, the
    samples of a chunk added in sample order from +0.0f.  Returns (chunk, g).  Cached per argument set; callers must not modify the array."""
    import oracle_binding as ob
    cam = camera if camera is not None else cornell.camera
    key = (id(cornell), w, h, spp, integrator, tuple(cam.pos), seed)
    if key not in _chunks:
        g = granule_of(spp)
        osc = ob.OracleScene(cornell.arrays, ob.MATH_PORTABLE)
        op = ob.make_params(w, h, spp, cam.as_dict(), seed=seed, integrator=integrator, sky=tuple(cornell.opt.scene_sky_default),
                            ibl_intensity=cornell.opt.IBL_intensity)
        chunk = np.zeros(((spp + g - 1) // g, h, w, 3, 3), f32)
        plane = np.zeros((h, w, 3, 3), f32)
        r, a, nn = ob.F3(), ob.F3(), ob.F3()
        sample = ob.lib().hjo_sample
        ctx, pp = osc.ctx, C.byref(op)
        for s in range(spp):
            for y in range(h):
                for x in range(w):
                    sample(ctx, pp, x, y, s, r, a, nn)
                    px = plane[y, x]
                    px[0], px[1], px[2] = r, a, nn
            chunk[s // g] = chunk[s // g] + plane
        chunk.setflags(write=False)
        _chunks[key] = (chunk, g)
    return _chunks[key]
