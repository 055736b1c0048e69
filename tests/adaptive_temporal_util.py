"""Adaptive sampling that counts the temporal history (option "adaptive_temporal"; include/henjou_hip.h, DESIGN.md §4 rule 11) restated in
numpy float32, and the native checker of its prior (tests/native/temporal_prior_ref.cpp).  No GPU needed; tools may import it.

Built on the butterfly of tests/test_gpu_adaptive.py::predict (rule 6) the way firefly_passes_util.py builds on it: every operation is one
IEEE fp32 operation in the order the header writes it, so the result equals the device's bit for bit.  `prior` None (or al = 1 everywhere)
is rule 6."""
import ctypes as C
import os
import subprocess

import numpy as np

from denoise_var_util import UNKNOWN, variance_rule
from firefly_util import f32, granule_of
from scene_util import hjr
from temporal_util import _side_bytes, build_checker, cam_floats

ADAPTIVE_EPS = f32(1e-3)  # HJR_ADAPTIVE_EPS
NO_PRIOR = np.array([0, 0, 1, 0], f32)  # what a pixel without a usable history carries


# ---- the prior
def prior_ref(prev, cur, n_tris):
    """The native checker of the prior on dicts as Device.temporal_prior takes them (cur: camera, transforms, inv_transforms, gbuffer,
    optionally coverage; prev as Device.temporal_accumulate's, or None): float32 [h, w, 4] = (lp, vp, al, 0)."""
    exe, tmp = build_checker("temporal_prior_ref")
    g = np.ascontiguousarray(cur["gbuffer"], hjr.GBUFFER_DTYPE)
    h, w = g.shape
    m = np.ascontiguousarray(cur["transforms"], f32).reshape(-1, 12)
    inv = np.ascontiguousarray(cur["inv_transforms"], f32).reshape(-1, 12)
    src, dst = os.path.join(tmp, "p_in.bin"), os.path.join(tmp, "p_out.bin")
    with open(src, "wb") as f:
        if prev is not None:
            f.write(_side_bytes(prev, True))
        f.write(cam_floats(cur["camera"]).tobytes() + m.tobytes() + inv.tobytes() + g.tobytes())
    subprocess.check_call([exe, str(w), str(h), str(m.shape[0]), str(int(n_tris)), "1" if prev is not None else "0",
                           str(int((prev or {}).get("coverage") or 0)), str(int(cur.get("coverage") or 0)), src, dst])
    raw = np.fromfile(dst, f32)
    assert raw.size == w * h * 4
    return raw.reshape(h, w, 4)


# ---- rule 11
def rule6_error(S1, S2, m, n):
    """Rule 6's per-pixel e from the raw statistic: m full chunks, n samples."""
    S1, S2 = np.asarray(S1, f32), np.asarray(S2, f32)
    m, n = f32(m), f32(n)
    with np.errstate(all="ignore"):
        q = np.maximum(m * S2 - S1 * S1, f32(0))
        return (np.sqrt(q / (m - f32(1))) / (S1 + ADAPTIVE_EPS * n)).astype(f32)


def variance_of_mean(S1, S2, m, g, n):
    """Rule 7's function on the statistic (csrc/hjr_aux.hip.h: hjr_variance_of_mean)."""
    S1, S2 = np.asarray(S1, f32), np.asarray(S2, f32)
    if m < 2:
        return np.full(S1.shape, UNKNOWN, f32)
    mf = f32(m)
    with np.errstate(all="ignore"):
        q = np.maximum(mf * S2 - S1 * S1, f32(0))
        return ((q / (mf * (mf - f32(1)))) / (f32(g) * f32(n))).astype(f32)


def rule11_error(S1, S2, g, n, prior):
    """Rule 11's per-pixel (e, e6) after n samples of granule g; prior [..., 4] = (lp, vp, al, 0) or None."""
    S1, S2 = np.asarray(S1, f32), np.asarray(S2, f32)
    m = n // g
    e6 = rule6_error(S1, S2, m, n)
    if prior is None:
        return e6, e6
    prior = np.asarray(prior, f32)
    lp, vp, al = prior[..., 0], prior[..., 1], prior[..., 2]
    with np.errstate(all="ignore"):
        lc = S1 / f32(n)
        vc = variance_of_mean(S1, S2, m, g, n)
        om = f32(1) - al
        va = (om * om) * vp + (al * al) * vc
        la = lp + (lc - lp) * al
        ea = np.sqrt(va) / (np.maximum(la, f32(0)) + ADAPTIVE_EPS)
        e = np.fmin(ea, e6)  # fminf: a NaN ea gives e6
    return np.where(al < f32(1), e, e6).astype(f32), e6


def butterfly(v):
    """The xor butterfly of a wave over 64 values: lane 0's sum."""
    v = np.asarray(v, f32).reshape(64).copy()
    idx = np.arange(64)
    for kx in (32, 16, 8, 4, 2, 1):
        v = v + v[idx ^ kx]
    return v[0]


def predict(chunk, g, w, h, spp, bounds, threshold, min_samples=0, prior=None):
    """Rule 11 (prior None: rule 6) for a frame rendered in the passes `bounds`.
    chunk: float32 [n_chunks][h][w][A][3], A = 1 (colour) or 3 (colour, albedo, normal) chunk sums of the whole frame; prior [h][w][4].
    Returns per pass a dict: n_tile uint32 [tiles_y][tiles_x] (samples each tile's mean is over), aovs (A frames [h][w][4]), variance
    float32 [h][w] (rule 7), active (tiles still active after the pass), decided (a deciding pass), sum / sum6 float32 [tiles_y][tiles_x]:
    the tile sums of rule 11 and of rule 6 on the same statistic for the tiles that decided at this pass (NaN elsewhere).  The frame ends
    with the pass that leaves no active tile: no later pass is in the list."""
    chunk = np.ascontiguousarray(chunk, f32)
    A = chunk.shape[3]
    col = chunk[:, :, :, 0, :]
    n_full = spp // g
    tx_n, ty_n = (w + 7) // 8, (h + 7) // 8
    H, W = ty_n * 8, tx_n * 8
    pad = np.zeros((chunk.shape[0], H, W, 3), f32)  # the butterfly runs over whole tiles: out-of-image lanes carry e = 0
    pad[:, :h, :w] = col
    pr = None
    if prior is not None:
        pr = np.broadcast_to(NO_PRIOR, (H, W, 4)).copy()
        pr[:h, :w] = np.asarray(prior, f32)
    inside = np.zeros((H, W), bool)
    inside[:h, :w] = True
    run = np.zeros((h, w, A, 3), f32)
    S1 = np.zeros((H, W), f32)
    S2 = np.zeros((H, W), f32)
    stopped = np.zeros((ty_n, tx_n), np.uint32)  # 0 = active, else n_tile
    ms = (min_samples + g - 1) // g * g if min_samples else 2 * g
    res = []
    for b, e in bounds:
        act = np.kron(stopped == 0, np.ones((8, 8), bool))
        for k in range(b // g, (e + g - 1) // g):
            run = np.where(act[:h, :w, None, None], run + chunk[k], run)
            if k < n_full:  # the statistic is over full chunks
                y = (pad[k][..., 0] + pad[k][..., 1]) + pad[k][..., 2]
                S1 = np.where(act, S1 + y, S1)
                S2 = np.where(act, S2 + y * y, S2)
        decided = threshold > 0 and e < spp and e >= ms and e // g >= 2
        sums = np.full((ty_n, tx_n), np.nan, f32)
        sums6 = np.full((ty_n, tx_n), np.nan, f32)
        if decided:
            err, err6 = rule11_error(S1, S2, g, e, pr)
            err = np.where(inside, err, f32(0)).astype(f32)
            err6 = np.where(inside, err6, f32(0)).astype(f32)
            for j in range(ty_n):
                for i in range(tx_n):
                    if stopped[j, i] == 0:
                        sums[j, i] = butterfly(err[8 * j:8 * j + 8, 8 * i:8 * i + 8])
                        sums6[j, i] = butterfly(err6[8 * j:8 * j + 8, 8 * i:8 * i + 8])
                        if sums[j, i] <= f32(threshold) * f32(64):
                            stopped[j, i] = e
        n_tile = np.where(stopped == 0, e, stopped).astype(np.uint32)
        n_px = np.kron(n_tile, np.ones((8, 8), np.uint32))[:h, :w]
        img = run * (f32(1) / n_px.astype(f32))[..., None, None]
        var = np.zeros((h, w), f32)
        for nv in sorted(set(int(v) for v in n_tile.reshape(-1))):  # a stopped tile: over its own chunks, n = n_tile
            sel = n_px == nv
            var[sel] = variance_rule(col[:, sel], g, nv // g, nv)
        out = np.ones((A, h, w, 4), f32)
        out[..., :3] = np.moveaxis(img, 2, 0)
        active = int((stopped == 0).sum())
        res.append({"n_tile": n_tile, "aovs": list(out), "variance": var, "active": active, "decided": decided, "sum": sums, "sum6": sums6, "bounds": (b, e)})
        if active == 0:
            break
    return res


# ---- the oracle's chunk sums of one frame of a sequence
_chunks = {}


def oracle_frame_chunks(cornell, arrays, key, w, h, spp, cam, frame, integrator=0, seed=1):
    """[n_chunks][h][w][3 AOVs][3] float32 chunk sums of the oracle's per-sample values of `frame` on the scene `arrays` (`key` names them
    in the cache), the samples of a chunk added in sample order from +0.0f.  Returns (chunk, g); callers must not modify the array."""
    import oracle_binding as ob
    cam = cam if isinstance(cam, dict) else cam.as_dict()
    ck = (key, w, h, spp, tuple(cam["pos"]), tuple(cam["dir"]), frame, integrator, seed)
    if ck not in _chunks:
        g = granule_of(spp)
        osc = ob.OracleScene(arrays, ob.MATH_PORTABLE)
        op = ob.make_params(w, h, spp, cam, frame=frame, seed=seed, integrator=integrator, sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)
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
        osc.close()
        chunk.setflags(write=False)
        _chunks[ck] = (chunk, g)
    return _chunks[ck]


# ---- a sequence on the CPU: the oracle's chunk sums, the native checkers' G-buffer, prior and accumulation, the restatement's decisions
def even_bounds(spp, step):
    return [(b, min(b + step, spp)) for b in range(0, spp, step)]


def cpu_sequence(cornell, w, h, spp, step, threshold, min_samples, frames, moved, cam, integrator=0, on=True, coverage=0):
    """Frames `frames` (their `frame` numbers; moved: None, or per frame the steps every instance is shifted by, temporal_util.moved_consistent) rendered in passes
    of `step` samples with rule 11 (on) or rule 6 (on False: the history still advances, as with the option on, so both arms see the same
    kind of frames) and accumulated without the filter, which no decision reads.  Yields per frame a dict: frame, arrays, geom (the current
    side without images), prev (the history the frame was decided against, None on the first), prior (None without history), pred (the
    restatement's passes), pred6 (rule 6 on the same chunk sums), hist (the history after the frame)."""
    import temporal_cov_util as tcu
    from temporal_util import moved_consistent, temporal_ref
    cam = cam if isinstance(cam, dict) else cam.as_dict()
    n_tris = np.asarray(cornell.arrays["indices"]).size // 3
    bounds = even_bounds(spp, step)
    prev = None
    for i, f in enumerate(frames):
        arrays = dict(cornell.arrays)
        k = moved[i] if moved else 0
        arrays["transforms"], arrays["inv_transforms"] = moved_consistent(cornell.arrays, k)
        chunk, g = oracle_frame_chunks(cornell, arrays, ("moved", k), w, h, spp, cam, f, integrator)
        gbuf = tcu.gbuffer_cov_ref(*tcu.rows_from_arrays(arrays), w, h, cam, coverage)
        geom = {"camera": cam, "transforms": np.asarray(arrays["transforms"], f32), "inv_transforms": np.asarray(arrays["inv_transforms"], f32), "gbuffer": gbuf}
        if coverage:
            geom["coverage"] = coverage
        prior = prior_ref(prev, geom, n_tris) if (on and prev is not None) else None
        pred = predict(chunk, g, w, h, spp, bounds, threshold, min_samples, prior)
        pred6 = predict(chunk, g, w, h, spp, bounds, threshold, min_samples, None)
        last = pred[-1]
        cur = dict(geom, color=last["aovs"][0], variance=last["variance"])
        acc = tcu.temporal_cov_ref(prev, cur, n_tris) if coverage else temporal_ref(prev, cur, n_tris)
        hist = dict(cur, color=acc[0], variance=acc[1], history=acc[2])
        yield {"frame": f, "arrays": arrays, "geom": geom, "prev": prev, "prior": prior, "pred": pred, "pred6": pred6, "hist": hist, "chunk": chunk, "g": g, "spp": spp, "step": step}
        prev = hist


def vacuity_counts(seq):
    """What the tests must not be vacuous about, counted over the frames of a cpu_sequence (or of the GPU test's own chain) that have a
    prior: tiles that stop strictly earlier than under rule 6; tiles that survive their first decision; restarted tiles (every pixel of the
    tile inside the image hits a surface and carries al = 1), which must take exactly rule 6's decisions: the same tile sums, bit for bit,
    at every deciding pass, and the same n_tile; and how many of those stop before spp.  Asserts property (b) on the way."""
    earlier = survive = restarted = restarted_stop = 0
    for fr in seq:
        if fr["prior"] is None:
            continue
        n11, n6 = fr["pred"][-1]["n_tile"], fr["pred6"][-1]["n_tile"]
        assert (n11 <= n6).all(), "property (b)"
        earlier += int((n11 < n6).sum())
        first = next(p for p in fr["pred"] if p["decided"])
        survive += first["active"]
        h, w = fr["prior"].shape[:2]
        rest = (fr["geom"]["gbuffer"]["prim"] != 0xffffffff) & (fr["prior"][..., 2] == 1)
        ty_n, tx_n = n11.shape
        for j in range(ty_n):
            for i in range(tx_n):
                if not rest[8 * j:8 * j + 8, 8 * i:8 * i + 8].all():  # (an edge tile: its pixels inside the image)
                    continue
                restarted += 1
                assert n11[j, i] == n6[j, i], "a restarted tile stops where rule 6 stops it"
                for p11, p6 in zip(fr["pred"], fr["pred6"]):
                    if p11["decided"] and not np.isnan(p6["sum6"][j, i]):
                        assert p11["sum"][j, i].view(np.uint32) == p6["sum6"][j, i].view(np.uint32), "a restarted tile's sum is rule 6's"
                restarted_stop += int(n6[j, i] < fr["pred6"][-1]["bounds"][1] or len(fr["pred6"]) < len(even_bounds(fr["spp"], fr["step"])))
    return {"earlier": earlier, "survive": survive, "restarted": restarted, "restarted_stop": restarted_stop}
