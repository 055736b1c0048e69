"""Shared by the guided-upscale tests and tools: the native checker of the rule (tests/native/upscale_guided_ref.cpp, built once per process
with g++ -O2 -ffp-contract=off; it restates the header comment of csrc/hjr_denoise.hip.h), a numpy float32 restatement of the plain bilinear
upscale, builders of synthetic and hostile G-buffers, and the quality comparison of DESIGN.md §11.4 on frames from any source (the CPU oracle
in tools/upscale_guided_rehearsal.py, the GPU in tests/test_gpu_upscale_guided.py and tools/upscale_guided_bench.py)."""
import os
import subprocess
import tempfile

import numpy as np

from scene_util import ROOT, hjr
from temporal_util import MISS, cam_floats, ref_mask

f32 = np.float32
_exe = None
_dir = None


def checker():
    global _exe, _dir
    if _exe is None:
        _dir = tempfile.TemporaryDirectory(prefix="hjr_ug_")
        exe = os.path.join(_dir.name, "upscale_guided_ref")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "upscale_guided_ref.cpp"), "-o", exe])
        _exe = exe
    return _exe


def upscale_guided_ref(color_lo, gbuffer_lo, cam, gbuffer_hi, k=None):
    """The native checker: (image [oh, ow, 4] float32, valid taps per pixel [oh, ow] int32).  k = (k_plane, k_normal) overrides the constants."""
    color_lo = np.ascontiguousarray(color_lo, f32)
    lo, hi = np.ascontiguousarray(gbuffer_lo, hjr.GBUFFER_DTYPE), np.ascontiguousarray(gbuffer_hi, hjr.GBUFFER_DTYPE)
    (ih, iw), (oh, ow) = lo.shape, hi.shape
    assert color_lo.shape == (ih, iw, 4) and ow // 2 == iw and oh // 2 == ih
    exe = checker()
    src, dst = os.path.join(_dir.name, "in.bin"), os.path.join(_dir.name, "out.bin")
    with open(src, "wb") as f:
        for a in (cam_floats(cam), color_lo, lo, hi):
            f.write(a.tobytes())
    cmd = [exe, str(iw), str(ih), str(ow), str(oh), src, dst]
    if k is not None:
        cmd += [repr(float(k[0])), repr(float(k[1]))]
    subprocess.check_call(cmd)
    raw = np.fromfile(dst, np.uint8)
    n = ow * oh
    assert raw.size == n * 20
    return raw[:n * 16].view(f32).reshape(oh, ow, 4), raw[n * 16:].view(np.int32).reshape(oh, ow)


def bilinear_np(color_lo, ow, oh):
    """hjr_upscale2x_kernel's expression in numpy float32: out = (a * gx + b * fx) * gy + (c * gx + d * fx) * fy per channel."""
    color_lo = np.asarray(color_lo, f32)
    ih, iw = color_lo.shape[:2]
    X, Y = np.arange(ow), np.arange(oh)
    x0, y0 = np.where(X % 2 == 1, X // 2, X // 2 - 1), np.where(Y % 2 == 1, Y // 2, Y // 2 - 1)
    fx = np.where(X % 2 == 1, f32(0.25), f32(0.75)).astype(f32)[None, :, None]
    fy = np.where(Y % 2 == 1, f32(0.25), f32(0.75)).astype(f32)[:, None, None]
    xa, xb = np.clip(x0, 0, iw - 1), np.clip(x0 + 1, 0, iw - 1)
    ya, yb = np.clip(y0, 0, ih - 1), np.clip(y0 + 1, 0, ih - 1)
    a, b, c, d = color_lo[ya][:, xa], color_lo[ya][:, xb], color_lo[yb][:, xa], color_lo[yb][:, xb]
    gx, gy = f32(1) - fx, f32(1) - fy
    return ((a * gx + b * fx) * gy + (c * gx + d * fx) * fy).astype(f32)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def changed_pixels(guided, bilinear):
    """[oh, ow] bool: some channel differs in bits."""
    return (bits(guided) != bits(bilinear)).any(axis=-1)


def all_miss(h, w):
    g = np.zeros((h, w), hjr.GBUFFER_DTYPE)
    g["prim"] = MISS
    return g


def hostile_gbuffer(h, w, seed):
    """Records a caller could hand over: random prim / inst words (misses and a few small instance ids among them, so that some taps do
    compare geometry), positions and normals from ordinary values, zeros, huge values, NaN and +-Inf."""
    rng = np.random.default_rng(seed)
    g = np.zeros((h, w), hjr.GBUFFER_DTYPE)
    words = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)
    kind = rng.integers(0, 4, (h, w))
    g["prim"] = np.where(kind == 0, np.uint32(MISS), words)
    g["inst"] = np.where(rng.integers(0, 3, (h, w)) == 0, rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32), np.uint32(1) + (kind == 3))
    special = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 3e38, -3e38, 1e-40, np.nan, np.inf, -np.inf], f32)
    for name in ("pos", "ng"):
        v = rng.normal(0, 1, (h, w, 3)).astype(f32)
        pick = rng.integers(0, 3, (h, w, 3)) == 0
        v[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
        g[name] = v
    g["t"], g["b1"], g["b2"] = (rng.normal(0, 1, (h, w)).astype(f32) for _ in range(3))
    g["pad"] = words[::-1, ::-1]
    return g


# ---- the quality comparison
QW, QH, Q_SPP, REF_SPP = 96, 64, 64, 4096  # output size; the render is QW / 2 x QH / 2 at Q_SPP, NEE, seed 1; reference at QW x QH, REF_SPP, seed 7


def _rmse(img, ref, sel):
    if not sel.any():
        return float("nan")
    return float(np.sqrt(np.mean((img[..., :3][sel].astype(np.float64) - ref[..., :3][sel]) ** 2)))


def quality_row(guided, bilinear, ref):
    """Errors against `ref` over its mask (light sources and background out): on the masked pixels the guided upscale changes, and on the
    whole mask; both arms come from the same filtered half-size image, so they differ in the changed pixels only."""
    mask = ref_mask(ref)
    changed = changed_pixels(guided, bilinear)
    sel = changed & mask
    return {"e_guided_changed": _rmse(guided, ref, sel), "e_bilinear_changed": _rmse(bilinear, ref, sel), "e_guided_mask": _rmse(guided, ref, mask),
            "e_bilinear_mask": _rmse(bilinear, ref, mask), "changed_share": float(changed.mean()), "changed_in_mask_share": float(sel.sum() / max(int(mask.sum()), 1)),
            "changed_in_mask": int(sel.sum()), "mask_share": float(mask.mean())}


def quality_conditions(table):
    """The asserted condition as (text, holds) pairs: on the row "x = 3.5", e_guided < e_bilinear over the masked pixels the upscale changes
    (no margin: both arms see the same samples).  Other rows (the scene's own camera) are reported only."""
    r = table["x = 3.5"]
    return [("x = 3.5, %d changed pixels in the mask: e_guided %.5f < e_bilinear %.5f" % (r["changed_in_mask"], r["e_guided_changed"], r["e_bilinear_changed"]),
             r["changed_in_mask"] > 0 and r["e_guided_changed"] < r["e_bilinear_changed"])]


def format_table(table):
    lines = ["camera        changed px (all / of mask)   RMSE on changed: bilinear  guided     RMSE on mask: bilinear  guided"]
    for name, r in table.items():
        lines.append("%-12s  %5.1f %% / %5.1f %%              %.5f   %.5f               %.5f   %.5f" % (
            name, 100 * r["changed_share"], 100 * r["changed_in_mask_share"], r["e_bilinear_changed"], r["e_guided_changed"], r["e_bilinear_mask"], r["e_guided_mask"]))
    return "\n".join(lines)


def gpu_quality_table(cornell, dev):
    """The rehearsal's frames on the GPU, every stage a library call: render QW / 2 x QH / 2 at Q_SPP with the variance AOV -> variance-guided
    filter (Denoise mode) -> the two G-buffers -> guided upscale; the bilinear arm is the 2x mode of the same filter call."""
    from temporal_util import camera_at
    kw = dict(sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)
    table = {}
    for name, cam in (("x = 3.5", camera_at(cornell, x=3.5)), ("scene camera", camera_at(cornell))):
        ref = dev.render(hjr.make_params(QW, QH, REF_SPP, cam, seed=7, **kw), want_aovs=False)[0]
        lo_p = hjr.make_params(QW // 2, QH // 2, Q_SPP, cam, seed=1, **kw)
        c, a, n, v = dev.render(lo_p, want_variance=True)
        filtered = dev.denoise(hjr.MODE_DENOISE, c, a, n, variance=v)
        bilinear = dev.denoise(hjr.MODE_DENOISE_UPSCALE2X, c, a, n, variance=v)
        guided = dev.upscale_guided(filtered, dev.gbuffer(lo_p), cam, dev.gbuffer(hjr.make_params(QW, QH, 1, cam)))
        table[name] = quality_row(guided, bilinear, ref)
    return table
