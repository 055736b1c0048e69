"""Shared by the temporal-accumulation tests: the native checker of the accumulation rule (tests/native/temporal_ref.cpp; it restates the
header comment of csrc/hjr_temporal.hip.h), the numpy float32 restatement of the pixel-centre ray, and small builders of frames (dicts of
arrays as Device.temporal_accumulate takes them).  And what the coverage, moments and response utilities beside it share: build_checker
(every native checker, built once per process with g++ -O2 -ffp-contract=off), same_bits, assert_same, luminance, next_prev."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from scene_util import ROOT, hjr

f32 = np.float32
UNKNOWN = f32(1e30)
MISS = 0xffffffff

_built = {}  # checker name -> (its temporary directory, the executable in it)


def build_checker(name):
    """tests/native/<name>.cpp, built once per process into a temporary directory of its own: (executable, that directory, where the
    caller keeps the checker's input and output files)."""
    if name not in _built:
        tmp = tempfile.TemporaryDirectory(prefix="hjr_%s_" % name)
        exe = os.path.join(tmp.name, name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe])
        _built[name] = (tmp, exe)
    tmp, exe = _built[name]
    return exe, tmp.name


def same_bits(a, b):
    """Bit equality of two float32 arrays (NaN payloads included)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_same(got, want, what, moments=False):
    """Two tuples of outputs of the accumulation agree bit for bit: colour, variance, history, then (moments) the moments, then lambda."""
    names = ("colour", "variance", "history") + (("moments",) if moments or (len(got) > 3 and np.ndim(got[3]) == 3) else ()) + ("lambda",)
    assert len(got) == len(want), (len(got), len(want))
    for name, g, w in zip(names, got, want):
        assert same_bits(g, w), "%s: %s differs in %d values" % (what, name, int(np.sum(np.ascontiguousarray(g, f32).view(np.uint32) != np.ascontiguousarray(w, f32).view(np.uint32))))


def luminance(color):
    c = np.asarray(color, f32)
    return (c[..., 0] + c[..., 1]) + c[..., 2]


def next_prev(cur, out, moments=False):
    """The next call's previous frame from this call's current one and its outputs (moments: out[3] holds them; a fourth output of shape
    [h, w, 2] is taken for them as well, so the callers that always accumulate moments need not say so)."""
    d = dict(cur, color=out[0], variance=out[1], history=out[2])
    if moments or (len(out) > 3 and np.ndim(out[3]) == 3):
        d["moments"] = out[3]
    return d


def cam_floats(cam):
    """Camera (ctypes or dict) -> 13 float32: pos, dir, up, right, f."""
    if not isinstance(cam, dict):
        cam = cam.as_dict()
    return np.array(list(cam["pos"]) + list(cam["dir"]) + list(cam["up"]) + list(cam["right"]) + [cam["f"]], f32)


def _side_bytes(d, with_history):
    g = np.ascontiguousarray(d["gbuffer"], hjr.GBUFFER_DTYPE)
    h, w = g.shape
    parts = [cam_floats(d["camera"]), np.ascontiguousarray(d["transforms"], f32).reshape(-1, 12), np.ascontiguousarray(d["inv_transforms"], f32).reshape(-1, 12), g,
             np.ascontiguousarray(d["color"], f32).reshape(h, w, 4), np.ascontiguousarray(d["variance"], f32).reshape(h, w)]
    if with_history:
        parts.append(np.ascontiguousarray(d["history"], f32).reshape(h, w))
    return b"".join(p.tobytes() for p in parts)


def temporal_ref(prev, cur, n_tris, k=None):
    """The native checker: (color [h, w, 4], variance [h, w], history [h, w]).  k = (k_plane, k_dist) overrides the constants."""
    exe, tmp = build_checker("temporal_ref")
    h, w = np.asarray(cur["gbuffer"]).shape
    n_inst = np.asarray(cur["transforms"], f32).size // 12
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        if prev is not None:
            f.write(_side_bytes(prev, True))
        f.write(_side_bytes(cur, False))
    cmd = [exe, str(w), str(h), str(n_inst), str(int(n_tris)), "1" if prev is not None else "0", src, dst]
    if k is not None:
        cmd += [repr(float(k[0])), repr(float(k[1]))]
    subprocess.check_call(cmd)
    raw = np.fromfile(dst, f32)
    assert raw.size == w * h * 6
    return raw[:w * h * 4].reshape(h, w, 4), raw[w * h * 4:w * h * 5].reshape(h, w), raw[w * h * 5:].reshape(h, w)


def centre_rays(w, h, cam):
    """numpy float32 restatement of the pixel-centre ray (hjr_classify_tiles_kernel's expressions): unit directions [h, w, 3]."""
    c = cam_floats(cam)
    pos, cd, cu, cr, f = c[0:3], c[3:6], c[6:9], c[9:12], c[12]
    W, H = f32(w), f32(h)
    px = np.arange(w, dtype=np.uint32).astype(f32)[None, :]
    py = np.arange(h, dtype=np.uint32).astype(f32)[:, None]
    u = np.broadcast_to((f32(2) * (px + f32(0.5)) - W) / H, (h, w))
    v = np.broadcast_to((f32(2) * (py + f32(0.5)) - H) / H, (h, w))
    d = [((cd[k] * f) + cr[k] * u) + cu[k] * v for k in range(3)]
    dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    inv = f32(1) / np.sqrt(dd)
    return np.stack([d[k] * inv for k in range(3)], axis=-1).astype(f32), pos


def identity_xf(n):
    m = np.zeros((n, 12), f32)
    m[:, 0] = m[:, 5] = m[:, 10] = 1
    return m


def translated(m, inv, t):
    """(M, M^-1) with the translation t added to M and the inverse updated consistently: inv_t' = inv_t - L^-1 t."""
    m, inv = np.array(m, f32).reshape(-1, 12).copy(), np.array(inv, f32).reshape(-1, 12).copy()
    t = np.asarray(t, f32)
    for r in range(3):
        m[:, 4 * r + 3] += t[r]
        inv[:, 4 * r + 3] -= (inv[:, 4 * r] * t[0] + inv[:, 4 * r + 1] * t[1]) + inv[:, 4 * r + 2] * t[2]
    return m, inv


def moved_consistent(arrays, k):
    """tests/test_device_bvh.py::moved (every instance shifted by k * (0.05, -0.03, 0.02)) with the inverses updated too."""
    return translated(arrays["transforms"], arrays["inv_transforms"], (f32(0.05 * k), f32(-0.03 * k), f32(0.02 * k)))


def wall_camera(x=0.0, y=0.0, f=2.0):
    """A camera at (x, y, 0) looking down -z with up = +y and right = +x (unit vectors)."""
    return {"pos": [x, y, 0.0], "dir": [0.0, 0.0, -1.0], "up": [0.0, 1.0, 0.0], "right": [1.0, 0.0, 0.0], "f": f}


def plane_gbuffer(w, h, cam, planes):
    """Synthetic G-buffer: `planes` is a list of (z, inst, prim, xmin, xmax) axis-aligned rectangles facing +z at depth z < 0 (world space,
    unbounded in y); the nearest one a pixel-centre ray hits wins; nothing hit = miss."""
    d, pos = centre_rays(w, h, cam)
    g = np.zeros((h, w), hjr.GBUFFER_DTYPE)
    g["prim"] = MISS
    best = np.full((h, w), np.inf)
    for z, inst, prim, xmin, xmax in planes:
        t = (f32(z) - pos[2]) / d[..., 2]
        p = pos[None, None, :] + d * t[..., None]
        hit = (t > 0) & (p[..., 0] >= xmin) & (p[..., 0] < xmax) & (t < best)
        best = np.where(hit, t, best)
        g["prim"][hit] = prim
        g["inst"][hit] = inst
        g["t"][hit] = t[hit]
        p[..., 2] = f32(z)
        g["pos"][hit] = p[hit].astype(f32)
        g["ng"][hit] = np.array([0, 0, 2], f32)
    return g


# ---- the quality comparison of tests/test_gpu_temporal.py, tools/temporal_rehearsal.py and tools/temporal_bench.py
def ref_mask(ref):
    """The mask rule of the variance filter's quality test: light sources out (a channel >= 3) and the constant background out (all
    channels within 1e-3 of the sky's 0.8)."""
    return (ref[..., :3].max(axis=-1) < 3.0) & (np.abs(ref[..., :3] - 0.8).max(axis=-1) > 1e-3)


def rmse(img, ref, mask):
    return float(np.sqrt(np.mean((img[..., :3][mask].astype(np.float64) - ref[..., :3][mask]) ** 2)))


def quality_table(refs, out_var, out_tmp):
    """Per-frame errors of the per-frame variance-guided filter and of the temporal path against each frame's reference (lists over the
    frames 1..n), and the flicker of both: mean over the masked pixels (of both frames) of |out_f - out_(f-1)|, averaged over f = 5..n."""
    masks = [ref_mask(r) for r in refs]
    t = {"e_var": [rmse(o, r, m) for o, r, m in zip(out_var, refs, masks)], "e_tmp": [rmse(o, r, m) for o, r, m in zip(out_tmp, refs, masks)],
         "mask_share": [float(m.mean()) for m in masks]}
    for key, outs in (("flicker_var", out_var), ("flicker_tmp", out_tmp)):
        d = [float(np.abs(outs[f][..., :3].astype(np.float64) - outs[f - 1][..., :3])[masks[f] & masks[f - 1]].mean()) for f in range(4, len(outs))]
        t[key] = float(np.mean(d))
    return t


def quality_conditions(t, static):
    """The issue's conditions on one sequence's table as (text, holds) pairs: e_tmp(8) < e_var(8) and mean e_tmp(4..8) < mean e_var(4..8);
    on the static sequence also e_tmp(8) < e_tmp(2) and less flicker."""
    ev, et = t["e_var"], t["e_tmp"]
    c = [("e_tmp(8) %.5f < e_var(8) %.5f" % (et[7], ev[7]), et[7] < ev[7]),
         ("mean e_tmp(4..8) %.5f < mean e_var(4..8) %.5f" % (np.mean(et[3:8]), np.mean(ev[3:8])), np.mean(et[3:8]) < np.mean(ev[3:8]))]
    if static:
        c.append(("e_tmp(8) %.5f < e_tmp(2) %.5f" % (et[7], et[1]), et[7] < et[1]))
        c.append(("flicker_tmp %.5f < flicker_var %.5f" % (t["flicker_tmp"], t["flicker_var"]), t["flicker_tmp"] < t["flicker_var"]))
    return c


def format_table(name, t):
    lines = ["%s   frame   e_var     e_tmp" % name]
    lines += ["%s   %5d   %.5f   %.5f" % (name, f + 1, a, b) for f, (a, b) in enumerate(zip(t["e_var"], t["e_tmp"]))]
    lines.append("%s   flicker (f = 5..8): per-frame filter %.5f, temporal %.5f" % (name, t["flicker_var"], t["flicker_tmp"]))
    return "\n".join(lines)


def camera_at(cornell, x=None, turn=0.0, shift=(0.0, 0.0, 0.0)):
    """The scene's camera, optionally moved to pos.x = x, shifted, and turned by `turn` radians about its up axis."""
    cam = hjr.Camera.from_buffer_copy(cornell.camera)
    if x is not None:
        cam.pos[0] = x
    for k in range(3):
        cam.pos[k] += shift[k]
    if turn:
        up = np.array(list(cam.up), np.float64)
        up /= np.linalg.norm(up)
        c, s = np.cos(turn), np.sin(turn)
        for name in ("dir", "right"):
            v = np.array(list(getattr(cam, name)), np.float64)
            r = v * c + np.cross(up, v) * s + up * np.dot(up, v) * (1 - c)
            setattr(cam, name, (C.c_float * 3)(*r))
    return cam


def quality_sequences(cornell, dev, w=96, h=64, spp=16, frames=8, ref_spp=4096):
    """The tables of sequence S (static) and M (instances moved by `frame` steps): per frame the error of the per-frame variance-guided
    filter (the parent's best, from the same renders) and of the temporal path, against a ref_spp render of that frame's geometry."""
    cam = camera_at(cornell, x=3.5)
    kw = dict(sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)
    tables = {}
    for name, static in (("S", True), ("M", False)):
        refs, out_var, out_tmp, prev = [], [], [], None
        for f in range(1, frames + 1):
            xf = moved_consistent(cornell.arrays, 0 if static else f)
            dev.set_transforms(*xf)
            if f == 1 or not static:
                ref = dev.render(hjr.make_params(w, h, ref_spp, cam, seed=7, **kw), want_aovs=False)[0]
            refs.append(ref)
            p = hjr.make_params(w, h, spp, cam, frame=f, seed=1, **kw)
            c, a, n, v = dev.render(p, want_variance=True)
            out_var.append(dev.denoise(hjr.MODE_DENOISE, c, a, n, variance=v))
            cur = {"camera": cam, "transforms": xf[0], "inv_transforms": xf[1], "gbuffer": dev.gbuffer(p), "color": c, "variance": v}
            tc, tv, th = dev.temporal_accumulate(prev, cur)
            out_tmp.append(dev.denoise(hjr.MODE_DENOISE, tc, a, n, variance=tv))
            prev = dict(cur, color=tc, variance=tv, history=th)
        tables[name] = quality_table(refs, out_var, out_tmp)
    return tables
