"""Shared by the tests of the windowed change test of the temporal accumulation (hjr_temporal_accumulate_response, option
"denoise_temporal_response") and by tools/temporal_response_rehearsal.py / tools/temporal_response_bench.py: the native
checker tests/native/temporal_response_ref.cpp (built once per process with g++ -O2 -ffp-contract=off; it restates sections ACCUMULATION,
COVERAGE-AWARE ACCUMULATION, TEMPORAL MOMENTS and RESPONSE of the header comment of csrc/hjr_temporal.hip.h), a numpy float32 restatement of
section RESPONSE alone, the three test sequences S, L and M, and the quality comparison of §11.8."""
import os
import subprocess

import numpy as np

from scene_util import hjr
from temporal_util import MISS, _side_bytes, build_checker, luminance, moved_consistent, next_prev, ref_mask, rmse, translated

f32 = np.float32
UNKNOWN = f32(1e30)
ALPHA = f32(0.2)
RESP_R, RESP_T0, RESP_T1, RESP_NMIN, RESP_EPS = 2, f32(3.0), f32(6.0), 5, f32(1e-3)

def temporal_response_ref(prev, cur, n_tris, moments=False, response=True, radius=None):
    """The native checker on dicts as Device.temporal_accumulate takes them (key "coverage" per side, absent = 0; prev["moments"] [h, w, 2]
    when moments): (color [h, w, 4], variance [h, w], history [h, w], moments [h, w, 2] if moments, lambda [h, w] if response)."""
    exe, tmp = build_checker("temporal_response_ref")
    h, w = np.asarray(cur["gbuffer"]).shape
    n_inst = np.asarray(cur["transforms"], f32).size // 12
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        if prev is not None:
            f.write(_side_bytes(prev, True))
            if moments:
                f.write(np.ascontiguousarray(prev["moments"], f32).reshape(h, w, 2).tobytes())
        f.write(_side_bytes(cur, False))
    cmd = [exe, str(w), str(h), str(n_inst), str(int(n_tris)), "1" if prev is not None else "0", str(int((prev or {}).get("coverage") or 0)),
           str(int(cur.get("coverage") or 0)), "1" if moments else "0", "1" if response else "0", src, dst]
    if radius is not None:
        cmd.append(str(int(radius)))
    subprocess.check_call(cmd)
    raw = np.fromfile(dst, f32)
    n = w * h
    assert raw.size == n * (6 + (2 if moments else 0) + (1 if response else 0))
    out = [raw[:n * 4].reshape(h, w, 4), raw[n * 4:n * 5].reshape(h, w), raw[n * 5:n * 6].reshape(h, w)]
    at = n * 6
    if moments:
        out.append(raw[at:at + 2 * n].reshape(h, w, 2))
        at += 2 * n
    if response:
        out.append(raw[at:].reshape(h, w))
    return tuple(out)


# ---- section RESPONSE alone, in numpy float32: every operation as written, the window in its order, one pixel image per window offset
def response_numpy(cur_color, c_prev, carried, gbuffer, n_tris, radius=RESP_R):
    """lambda [h, w] from the current colour, every pixel's c_prev ([h, w, 3]; looked at where carried only), the carried mask and the
    current G-buffer."""
    lc, lp = luminance(cur_color), luminance(c_prev)
    g = np.asarray(gbuffer)
    h, w = lc.shape
    ok = carried & (g["prim"] != MISS) & (g["prim"] < n_tris)
    inst = g["inst"]
    zero = np.zeros((h, w), f32)
    Sd, Sc, Sc2, n = zero.copy(), zero.copy(), zero.copy(), np.zeros((h, w), np.int64)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                member = inside & ok[qy, qx] & (inst[qy, qx] == inst)
                d = lc[qy, qx] - lp[qy, qx]
                Sd = np.where(member, Sd + d, Sd)
                Sc = np.where(member, Sc + lc[qy, qx], Sc)
                Sc2 = np.where(member, Sc2 + lc[qy, qx] * lc[qy, qx], Sc2)
                n += member
        nf = n.astype(f32)
        mu_d, mu_c = Sd / nf, Sc / nf
        var_c = Sc2 / nf - mu_c * mu_c
        var_c = np.where(var_c > 0, var_c, f32(0))  # fmaxf(x, 0): a NaN gives 0
        se = np.sqrt(var_c / nf) + RESP_EPS
        t = np.abs(mu_d) / se
        lam = (t - RESP_T0) / (RESP_T1 - RESP_T0)
        lam = np.where(lam > 0, lam, f32(0))
        lam = np.where(lam < 1, lam, f32(1))
    return np.where(carried & (n >= RESP_NMIN), lam, f32(0)).astype(f32)


def blend_numpy(cur_color, cur_var, c_prev, v_prev, h_prev, carried, lam):
    """Step 4 with al' = fmaxf(al, lambda) (no moments, every variance known): colour, variance, history."""
    with np.errstate(all="ignore"):
        hh = np.minimum(np.maximum(h_prev + f32(1), f32(1)), f32(64))
        al = np.maximum(f32(1) / hh, ALPHA)
        al = np.maximum(al, lam)
        hh = np.where(lam > 0, np.minimum(hh, f32(1) / al), hh)
        col = np.array(cur_color, f32)
        for c in range(3):
            col[..., c] = np.where(carried, c_prev[..., c] + (cur_color[..., c] - c_prev[..., c]) * al, cur_color[..., c])
        om = f32(1) - al
        var = np.where(carried, (om * om) * v_prev + (al * al) * np.maximum(cur_var, f32(0)), cur_var)
    return col.astype(f32), var.astype(f32), np.where(carried, hh, f32(1)).astype(f32)


# ---- the synthetic planes case (host and GPU tests): 37 x 19, so the kernel's 16 x 16 tiles are ragged and a window spans four workgroups
PW, PH, P_SPLIT, P_TRIS = 37, 19, 18, 12
P_NOISE, P_RAISE = f32(0.0625), f32(0.0875)  # the current luminance is history + raise +- noise (a checkerboard): t = raise sqrt(n) / noise
P_ISLAND4 = [(28, 4), (29, 4), (28, 5), (29, 5)]             # (x, y): instance 2, n = 4 < NMIN
P_ISLAND5 = [(30, 12), (29, 12), (31, 12), (30, 11), (30, 13)]  # instance 3, n = 5
P_MISS = (slice(0, 4), slice(33, 37))                        # rows, columns


def planes_case(seed=1):
    """Two wall instances that meet between columns 17 and 18 (instance 0 left, 1 right), a 2 x 2 island of instance 2 and a plus-shaped
    island of five pixels of instance 3 inside the right one, a miss block in the top right corner; identity transforms and one camera, so
    every hit pixel is carried.  The history is constant per instance (powers of two: c_prev, v_prev and h_prev come back exactly, whatever
    the bilinear weights are: h_prev = 8, v_prev = 2^-6), the current colour is the history plus a +-P_NOISE checkerboard in red (and a
    jitter of 1e-4), raised by P_RAISE on instance 0 and by 1 on the islands.  With n members t = raise sqrt(n) / noise (EPS aside):
    7 at n = 25, 6.3 at n = 20 (lambda = 1), 5.4 at n = 15 (the column beside the split and the image's edge columns and rows: partial),
    4.2 in the corners; on the right the window mean of the checkerboard is at most noise / n: t < 0.3, lambda = 0.
    Returns (prev, cur, c_prev [h, w, 3])."""
    from temporal_util import identity_xf, plane_gbuffer, wall_camera
    cam = wall_camera()
    g = plane_gbuffer(PW, PH, cam, [(-4.0, 0, 7, -1e9, -0.1), (-4.0, 1, 3, -0.1, 1e9)])
    assert (g["inst"][:, :P_SPLIT] == 0).all() and (g["inst"][:, P_SPLIT:] == 1).all()
    for x, y in P_ISLAND4:
        g["inst"][y, x] = 2
    for x, y in P_ISLAND5:
        g["inst"][y, x] = 3
    miss = np.zeros((), hjr.GBUFFER_DTYPE)
    miss["prim"] = MISS
    g[P_MISS] = miss
    const = np.array([[0.25, 0.125, 0.125], [0.5, 0.25, 0.25], [0.125, 0.125, 0.25], [1.0, 0.5, 0.5]], f32)
    c_prev = const[np.minimum(g["inst"], 3)]
    rng = np.random.default_rng(seed)
    prev_color = np.concatenate([c_prev, rng.uniform(0, 1, (PH, PW, 1)).astype(f32)], axis=-1)
    ys, xs = np.mgrid[0:PH, 0:PW]
    checker = np.where((xs + ys) % 2 == 0, P_NOISE, -P_NOISE).astype(f32)
    raise_ = np.select([g["inst"] == 0, g["inst"] >= 2], [P_RAISE, f32(1.0)], f32(0.0)).astype(f32)
    cur_color = prev_color.copy()
    cur_color[..., 0] = c_prev[..., 0] + raise_ + checker + rng.uniform(-1e-4, 1e-4, (PH, PW)).astype(f32)
    cur_color[..., 3] = rng.uniform(0, 1, (PH, PW)).astype(f32)
    xf = identity_xf(4)
    prev = {"camera": cam, "transforms": xf, "inv_transforms": xf, "gbuffer": g, "color": prev_color, "variance": np.full((PH, PW), 2.0 ** -6, f32),
            "history": np.full((PH, PW), 8.0, f32)}
    cur = {"camera": cam, "transforms": xf, "inv_transforms": xf, "gbuffer": g.copy(), "color": cur_color, "variance": rng.uniform(0.01, 0.02, (PH, PW)).astype(f32)}
    return prev, cur, c_prev


# ---- the staging case of the host entry points (GPU tests of hjr_temporal_accumulate_response and hjr_temporal_prior)
def staging_case(seed=11):
    """7 x 5 pixels of three wall instances side by side, seen by two cameras a fifth of a unit apart: 35 pixels, so the one-float images
    are an odd number of floats and the float2 and float4 images staged behind them start on their own alignment only if the host entry
    point's layout puts them there; three instances, so M and M^-1 are 36 floats each.  Returns (prev with moments, cur)."""
    from temporal_util import identity_xf, plane_gbuffer, wall_camera
    w, h = 7, 5
    planes = [(-4.0, 0, 1, -1e9, -0.6), (-4.0, 1, 2, -0.6, 0.6), (-4.0, 2, 3, 0.6, 1e9)]
    rng = np.random.default_rng(seed)
    side = lambda cam: {"camera": cam, "transforms": identity_xf(3), "inv_transforms": identity_xf(3), "gbuffer": plane_gbuffer(w, h, cam, planes),
                        "color": rng.uniform(0.1, 0.9, (h, w, 4)).astype(f32), "variance": rng.uniform(0.01, 0.02, (h, w)).astype(f32)}
    prev, cur = side(wall_camera()), side(wall_camera(x=0.2))
    assert all((g["inst"] == k).any() for g in (prev["gbuffer"], cur["gbuffer"]) for k in range(3))
    prev["history"] = rng.integers(1, 9, (h, w)).astype(f32)
    prev["moments"] = rng.uniform(0.1, 0.9, (h, w, 2)).astype(f32)
    return prev, cur


def check_planes_lambda(lam, what):
    """The lambda image of planes_case: what the construction gives (docstring of planes_case)."""
    assert (lam[2:PH - 2, 2:P_SPLIT - 2] == 1).all(), what + ": the raised instance's interior"
    right = np.ones((PH, PW), bool)
    right[:, :P_SPLIT] = False
    for x, y in P_ISLAND4 + P_ISLAND5:
        right[y, x] = False
    assert (lam[right] == 0).all(), what + ": the right instance and the miss block"
    col = lam[2:PH - 2, P_SPLIT - 1]
    assert ((col > 0) & (col < 1)).all(), what + ": the column beside the split (n = 15) answers partially"
    assert ((lam[2:PH - 2, 0] > 0) & (lam[2:PH - 2, 0] < 1)).all() and 0 < lam[0, 0] < lam[2, 0], what + ": windows cut by the image's edge"
    assert all(lam[y, x] == 0 for x, y in P_ISLAND4), what + ": four members are too few"
    assert all(lam[y, x] == 1 for x, y in P_ISLAND5), what + ": five members answer"


# ---- the sequences of §11.8: S static, L only the instance that holds the light moves (from frame 4 on), M every instance moves
QFRAMES = 10


def light_instance(arrays):
    """The instance that holds the first light primitive (instance 1 of cornelbox.gltf)."""
    po = np.asarray(arrays["prim_offsets"]).reshape(-1).astype(np.int64)
    return int(np.searchsorted(po, int(np.asarray(arrays["light_prim_ids"]).reshape(-1)[0]), side="right") - 1)


def sequence_transforms(arrays, seq, f):
    """(transforms, inverse transforms) of frame f (1-based) of sequence "S", "L" or "M"."""
    if seq == "M":
        return moved_consistent(arrays, f)
    m, inv = moved_consistent(arrays, 0)
    if seq == "L":
        k = light_instance(arrays)
        m[k:k + 1], inv[k:k + 1] = translated(m[k:k + 1], inv[k:k + 1], (f32(0.12 * max(0, f - 3)), f32(0), f32(0)))
    return m, inv


def geometry_changes(seq, f):
    """Whether frame f of the sequence has another geometry than frame f - 1 (a new reference and G-buffer are due)."""
    return f == 1 or seq == "M" or (seq == "L" and f >= 4)


def quality_chain(frames, refs, accumulate, denoise):
    """frames: per frame a dict with the keys of a temporal frame plus "albedo", "normal".  accumulate(prev, cur, response) -> 3 or 4
    arrays, denoise(color, albedo, normal, variance) -> image: the stages, from the GPU or from the native checkers.  Returns the table
    {"e_var", "e_tmp", "e_resp": [rmse per frame], "share": [share of pixels with lambda > 0 per frame], "out_resp": the last column's images}."""
    masks = [ref_mask(r) for r in refs]
    t = {"e_var": [rmse(denoise(fr["color"], fr["albedo"], fr["normal"], fr["variance"]), r, m) for fr, r, m in zip(frames, refs, masks)]}
    for key, response in (("e_tmp", False), ("e_resp", True)):
        prev, errs, outs, share = None, [], [], []
        for fr, ref, mask in zip(frames, refs, masks):
            cur = {k: fr[k] for k in ("camera", "transforms", "inv_transforms", "gbuffer", "color", "variance")}
            out = accumulate(prev, cur, response)
            outs.append(denoise(out[0], fr["albedo"], fr["normal"], out[1]))
            errs.append(rmse(outs[-1], ref, mask))
            if response:
                share.append(float((out[3] > 0).mean()))
            prev = next_prev(cur, out)
        t[key] = errs
        t["out_" + key[2:]] = outs
        if response:
            t["share"] = share
    for key in ("tmp", "resp"):
        outs = t["out_" + key]
        d = [float(np.abs(outs[f][..., :3].astype(np.float64) - outs[f - 1][..., :3])[masks[f] & masks[f - 1]].mean()) for f in range(4, 8)]
        t["flicker_" + key] = float(np.mean(d))
    outs = [denoise(fr["color"], fr["albedo"], fr["normal"], fr["variance"]) for fr in frames[3:8]]
    t["flicker_var"] = float(np.mean([float(np.abs(outs[i][..., :3].astype(np.float64) - outs[i - 1][..., :3])[masks[3 + i] & masks[2 + i]].mean()) for i in range(1, 5)]))
    return t


def mean410(e):
    return float(np.mean(e[3:10]))


def quality_conditions(tables, size=(96, 64)):
    """The conditions of §11.8 on {"S": table, "L": table}: (text, holds, asserted) triples.  L's two conditions against e_tmp are asserted
    at 48 x 32, the size the plain temporal path loses frames at; at 96 x 64 it does not (e_tmp(4) 0.0437 against e_var(4) 0.0471 in the
    rehearsal, with R = 2 and with the one re-tune R = 3), so no rule can halve it: there they are reported, as §11.2 did with M."""
    cond = []
    t = tables.get("L")
    if t:
        ev, et, er = mean410(t["e_var"]), mean410(t["e_tmp"]), mean410(t["e_resp"])
        against_tmp = tuple(size) == (48, 32)
        cond.append(("L mean e_resp(4..10) %.5f < mean e_var(4..10) %.5f" % (er, ev), er < ev, True))
        cond.append(("L mean e_resp(4..10) %.5f < 0.75 x mean e_tmp(4..10) %.5f" % (er, et), er < 0.75 * et, against_tmp))
        cond.append(("L e_resp(4) %.5f < 0.5 x e_tmp(4) %.5f" % (t["e_resp"][3], t["e_tmp"][3]), t["e_resp"][3] < 0.5 * t["e_tmp"][3], against_tmp))
    t = tables.get("S")
    if t:
        et, er = mean410(t["e_tmp"]), mean410(t["e_resp"])
        cond.append(("S mean e_resp(4..10) %.5f <= 1.02 x mean e_tmp(4..10) %.5f" % (er, et), er <= 1.02 * et, True))
        ev, e = t["e_var"], t["e_resp"]  # §11.2's four conditions on S with e_resp in place of e_tmp
        cond.append(("S e_resp(8) %.5f < e_var(8) %.5f" % (e[7], ev[7]), e[7] < ev[7], True))
        cond.append(("S mean e_resp(4..8) %.5f < mean e_var(4..8) %.5f" % (np.mean(e[3:8]), np.mean(ev[3:8])), np.mean(e[3:8]) < np.mean(ev[3:8]), True))
        cond.append(("S e_resp(8) %.5f < e_resp(2) %.5f" % (e[7], e[1]), e[7] < e[1], True))
        cond.append(("S flicker_resp %.5f < flicker_var %.5f" % (t["flicker_resp"], t["flicker_var"]), t["flicker_resp"] < t["flicker_var"], True))
    return cond


def format_tables(tables):
    lines = []
    for seq in sorted(tables):
        t = tables[seq]
        lines.append("%s   frame   e_var     e_tmp     e_resp    lambda > 0" % seq)
        for f in range(len(t["e_var"])):
            lines.append("%s   %5d   %.5f   %.5f   %.5f   %5.1f %%" % (seq, f + 1, t["e_var"][f], t["e_tmp"][f], t["e_resp"][f], 100 * t["share"][f]))
        lines.append("%s   mean(4..10)   %.5f   %.5f   %.5f" % (seq, mean410(t["e_var"]), mean410(t["e_tmp"]), mean410(t["e_resp"])))
        lines.append("%s   flicker (f = 5..8): per-frame filter %.5f, temporal %.5f, with response %.5f" % (seq, t["flicker_var"], t["flicker_tmp"], t["flicker_resp"]))
    return "\n".join(lines)


def worst_pixels(img, ref, mask, n=10):
    """The n masked pixels of the largest squared error: lines "x y error"."""
    e = ((img[..., :3].astype(np.float64) - ref[..., :3]) ** 2).sum(axis=-1) * mask
    idx = np.argsort(e.reshape(-1))[::-1][:n]
    return ["x %3d y %3d  err %.4f" % (int(i % e.shape[1]), int(i // e.shape[1]), float(np.sqrt(e.reshape(-1)[i] / 3))) for i in idx]
