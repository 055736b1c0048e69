#!/usr/bin/env python3
"""tools/adaptive_temporal_rehearsal.py [--size 48x32] [--frames 4] [--spp 64] [--step 16] [--threshold 0.08] [--min-samples 16] [--ref-spp 1024] [--sequences SM]
CPU rehearsal of the quality and saving comparison of option "adaptive_temporal" (tools/adaptive_temporal_bench.py):
no GPU, every stage from a CPU restatement, in the pattern of tools/temporal_rehearsal.py.

  frames     the CPU oracle's chunk sums (NEE, seed 1, `frame` advancing, camera at x = 3.5); sequence S static, sequence M every instance
             moved by frame * (0.05, -0.03, 0.02)
  G-buffer   tests/native/temporal_cov_ref.cpp's brute-force pass (side 0)
  stages     tests/adaptive_temporal_util.py (rules 6 and 11), tests/native/temporal_prior_ref.cpp (prior), tests/native/temporal_ref.cpp
             (accumulation), tests/native/denoise_var_ref.cpp (variance-guided filter)
  reference  the oracle at --ref-spp samples, seed 7, of each frame's geometry (one for S, one per frame for M); the mask of §11.2
  arms       adaptive   rule 6 without a history, filtered per frame           (adaptive sampling as it was)
             temporal   every frame at full spp, accumulated, filtered         (temporal accumulation as it was)
             both       rule 11 against the history, accumulated, filtered     (the new option)
Prints per frame the share of the frame's samples each arm rendered and the RMSE of its filtered output."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adaptive_temporal_util as atu  # noqa: E402
import oracle_binding as ob  # noqa: E402
from denoise_var_util import denoise_var_ref, variance_rule  # noqa: E402
from scene_util import Cornell  # noqa: E402
from temporal_util import camera_at, moved_consistent, ref_mask, rmse, temporal_ref  # noqa: E402

f32 = np.float32


def rehearse(cornell, w, h, frames, spp, step, threshold, min_samples, ref_spp, sequences="SM"):
    """{sequence: {arm: {"share": [...], "rmse": [...]}}} over frames 1..frames."""
    cam = camera_at(cornell, x=3.5).as_dict()
    n_tris = np.asarray(cornell.arrays["indices"]).size // 3
    sky = dict(sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)
    res = {}
    for name in sequences:
        static = name == "S"
        fr_ids = tuple(range(1, frames + 1))
        moved = None if static else fr_ids
        t = {arm: {"share": [], "rmse": []} for arm in ("adaptive", "temporal", "both")}
        prev_full, ref = None, None
        for fr in atu.cpu_sequence(cornell, w, h, spp, step, threshold, min_samples, fr_ids, moved, cam):
            if ref is None or not static:
                osc = ob.OracleScene(fr["arrays"], ob.MATH_PORTABLE)
                ref = osc.render(ob.make_params(w, h, ref_spp, cam, frame=1, seed=7, **sky))[0]
                osc.close()
            mask = ref_mask(ref)
            tiles = fr["pred"][-1]["n_tile"].size
            # adaptive sampling alone
            last6 = fr["pred6"][-1]
            c, al, n = last6["aovs"]
            t["adaptive"]["share"].append(float(last6["n_tile"].sum()) / (tiles * spp))
            t["adaptive"]["rmse"].append(rmse(denoise_var_ref(1, c, al, n, last6["variance"])[0], ref, mask))
            # temporal accumulation at full spp
            chunk, g = fr["chunk"], fr["g"]
            full = atu.predict(chunk, g, w, h, spp, [(0, spp)], 0.0)[-1]
            cur = dict(fr["geom"], color=full["aovs"][0], variance=variance_rule(chunk[:, :, :, 0, :], g, spp // g, spp))
            tc, tv, th = temporal_ref(prev_full, cur, n_tris)
            prev_full = dict(cur, color=tc, variance=tv, history=th)
            t["temporal"]["share"].append(1.0)
            t["temporal"]["rmse"].append(rmse(denoise_var_ref(1, tc, full["aovs"][1], full["aovs"][2], tv)[0], ref, mask))
            # both: rule 11
            last = fr["pred"][-1]
            t["both"]["share"].append(float(last["n_tile"].sum()) / (tiles * spp))
            t["both"]["rmse"].append(rmse(denoise_var_ref(1, fr["hist"]["color"], last["aovs"][1], last["aovs"][2], fr["hist"]["variance"])[0], ref, mask))
            print("%s frame %d: share %.3f / 1.000 / %.3f, rmse %.5f / %.5f / %.5f" % (name, fr["frame"], t["adaptive"]["share"][-1], t["both"]["share"][-1],
                                                                                        t["adaptive"]["rmse"][-1], t["temporal"]["rmse"][-1], t["both"]["rmse"][-1]), flush=True)
        res[name] = t
    return res


def format_tables(res):
    lines = []
    for name, t in res.items():
        lines.append("%s  frame  adaptive: share rmse    temporal: share rmse    both: share rmse" % name)
        for f in range(len(t["both"]["share"])):
            lines.append("%s  %5d  %.3f %.5f           %.3f %.5f           %.3f %.5f" % (name, f + 1, t["adaptive"]["share"][f], t["adaptive"]["rmse"][f], t["temporal"]["share"][f],
                                                                                 t["temporal"]["rmse"][f], t["both"]["share"][f], t["both"]["rmse"][f]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="48x32")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--step", type=int, default=16)
    ap.add_argument("--threshold", type=float, default=0.08)
    ap.add_argument("--min-samples", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--sequences", default="SM")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    w, h = map(int, a.size.split("x"))
    res = rehearse(Cornell(), w, h, a.frames, a.spp, a.step, a.threshold, a.min_samples, a.ref_spp, a.sequences)
    print(format_tables(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
