"""Shared by the tests of the temporal luminance moments (hjr_temporal_accumulate_moments, option "denoise_temporal_moments"; DESIGN.md
§11.7) and by tools/temporal_moments_rehearsal.py / tools/temporal_moments_bench.py: the native checker tests/native/temporal_moments_ref.cpp
(built once per process with g++ -O2 -ffp-contract=off; it restates sections ACCUMULATION, COVERAGE-AWARE ACCUMULATION and TEMPORAL MOMENTS of
the header comment of csrc/hjr_temporal.hip.h), the chain of stateless stages that option chains in the context, and the quality
comparison of §11.7."""
import os
import subprocess

import numpy as np

from temporal_util import _side_bytes, build_checker, ref_mask, rmse

f32 = np.float32
UNKNOWN = f32(1e30)
MOMENTS_MIN = f32(4.0)
K_LIMIT = f32(0.2) / (f32(2.0) - f32(0.2))  # HJR_TEMPORAL_ALPHA / (2 - HJR_TEMPORAL_ALPHA)

def temporal_moments_ref(prev, cur, n_tris, moments=True, moments_min=None):
    """The native checker on dicts as Device.temporal_accumulate takes them (key "coverage" per side, absent = 0; prev["moments"] [h, w, 2]
    when moments): (color [h, w, 4], variance [h, w], history [h, w], moments [h, w, 2]); without moments the first three."""
    exe, tmp = build_checker("temporal_moments_ref")
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
           str(int(cur.get("coverage") or 0)), "1" if moments else "0", src, dst]
    if moments_min is not None:
        cmd.append(repr(float(moments_min)))
    subprocess.check_call(cmd)
    raw = np.fromfile(dst, f32)
    n = w * h
    assert raw.size == n * (8 if moments else 6)
    out = (raw[:n * 4].reshape(h, w, 4), raw[n * 4:n * 5].reshape(h, w), raw[n * 5:n * 6].reshape(h, w))
    return out + (raw[n * 6:].reshape(h, w, 2),) if moments else out


# ---- the quality comparison of §11.7: per-frame RMSE of filter(temporal path) against the frame's reference, four ways
#   "spatial"           temporal accumulation behind the 3 x 3 spatial estimate (the parent's best at <= 8 spp)
#   "spatial+moments"   the same with the moments
#   "unknown"           temporal accumulation alone at <= 8 spp: the variance stays unknown
#   "moments"           the moments without the spatial estimate
WAYS = (("spatial", True, False), ("spatial+moments", True, True), ("unknown", False, False), ("moments", False, True))


def quality_chain(frames, refs, accumulate, estimate, denoise):
    """frames: per frame a dict with the keys of a temporal frame plus "albedo", "normal" (its variance as rendered).  accumulate(prev, cur,
    moments) -> 3 or 4 arrays, estimate(color, albedo, normal, variance) -> variance, denoise(color, albedo, normal, variance) -> image:
    the stages, from the GPU or from the native checkers.  Returns {way: [rmse per frame]}."""
    masks = [ref_mask(r) for r in refs]
    table = {}
    for way, spatial, moments in WAYS:
        prev, errs = None, []
        for fr, ref, mask in zip(frames, refs, masks):
            cur = {k: fr[k] for k in ("camera", "transforms", "inv_transforms", "gbuffer", "color")}
            cur["variance"] = estimate(fr["color"], fr["albedo"], fr["normal"], fr["variance"]) if spatial else fr["variance"]
            out = accumulate(prev, cur, moments)
            errs.append(rmse(denoise(out[0], fr["albedo"], fr["normal"], out[1]), ref, mask))
            prev = dict(cur, color=out[0], variance=out[1], history=out[2])
            if moments:
                prev["moments"] = out[3]
        table[way] = errs
    return table


def quality_conditions(tables):
    """The asserted conditions of the issue on {(sequence, spp): table}: (text, holds) pairs."""
    cond = []
    for spp in (4, 8):
        t = tables.get(("static", spp))
        if t:
            for f in range(3, 8):
                cond.append(("static %d spp frame %d: spatial+moments %.5f < spatial %.5f" % (spp, f + 1, t["spatial+moments"][f], t["spatial"][f]),
                             t["spatial+moments"][f] < t["spatial"][f]))
    for spp in (4, 8):
        t = tables.get(("static", spp))
        if t:
            for f in range(4, 8):
                cond.append(("static %d spp frame %d: moments %.5f < unknown %.5f" % (spp, f + 1, t["moments"][f], t["unknown"][f]), t["moments"][f] < t["unknown"][f]))
    for spp in (4, 8):
        t = tables.get(("moving", spp))
        if t:
            a, b = float(np.mean(t["spatial+moments"][4:8])), float(np.mean(t["spatial"][4:8]))
            cond.append(("moving %d spp mean(5..8): spatial+moments %.5f <= 1.02 x spatial %.5f" % (spp, a, b), a <= 1.02 * b))
    return cond


def format_tables(tables):
    lines = []
    for (seq, spp), t in sorted(tables.items()):
        lines.append("%s, %d spp   frame   spatial   spatial+moments   unknown   moments" % (seq, spp))
        for f in range(len(t["spatial"])):
            lines.append("%s, %d spp   %5d   %.4f    %.4f            %.4f    %.4f" % (seq, spp, f + 1, t["spatial"][f], t["spatial+moments"][f], t["unknown"][f], t["moments"][f]))
        lines.append("%s, %d spp   mean(5..8)   %.4f    %.4f            %.4f    %.4f" % ((seq, spp) + tuple(float(np.mean(t[k][4:8])) for k in ("spatial", "spatial+moments", "unknown", "moments"))))
    return "\n".join(lines)
