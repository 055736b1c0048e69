#!/usr/bin/env python3
"""tools/temporal_moments_rehearsal.py [--size 96x64] [--ref-spp 4096] [--spps 1,4,8] [--moments-min 4]
CPU rehearsal of the quality comparison of tests/test_gpu_temporal_moments.py: no GPU, every stage from a CPU restatement.

  frames     the CPU oracle (oracle/), NEE, seed 1, camera at x = 3.5; frames 1..8 with `frame` advancing at each of --spps; static, and every
             instance moved by frame * (0.05, -0.03, 0.02).  Every such frame is a single chunk: its variance AOV is unknown everywhere
  G-buffer   tools/temporal_rehearsal.gbuffer_cpu (the oracle's brute-force closest hit of the pixel-centre rays)
  stages     tests/native/spatial_var_ref.cpp (the 3 x 3 estimate), tests/native/temporal_moments_ref.cpp (accumulation, with and without
             the moments), tests/native/denoise_var_ref.cpp (variance-guided filter)
  reference  the oracle at --ref-spp samples, seed 7, of each frame's geometry; the mask of §11.2
Four columns per sequence and spp: the temporal path behind the spatial estimate (the best without moments), the same with moments, the
temporal path alone (variance unknown for ever) and the moments alone.  Prints the tables and the asserted conditions of the GPU test
(those of 4 and 8 spp; 1 spp is printed only); exit status 1 if one fails."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_binding as ob  # noqa: E402
from denoise_var_util import denoise_var_ref  # noqa: E402
from scene_util import Cornell, hjr  # noqa: E402
from spatial_var_util import spatial_var_ref  # noqa: E402
from temporal_moments_util import format_tables, quality_chain, quality_conditions, temporal_moments_ref  # noqa: E402
from temporal_rehearsal import cornell_params, gbuffer_cpu  # noqa: E402
from temporal_util import moved_consistent  # noqa: E402

FRAMES = 8


def rehearse(cornell, w, h, ref_spp, spps=(1, 4, 8), moments_min=None, log=None):
    """{(sequence, spp): table} of the CPU oracle's frames."""
    cam = hjr.Camera.from_buffer_copy(cornell.camera)
    cam.pos[0] = 3.5
    cam = cam.as_dict()
    n_tris = np.asarray(cornell.arrays["indices"]).size // 3
    log = log or (lambda s: None)
    accumulate = lambda prev, cur, moments: temporal_moments_ref(prev, cur, n_tris, moments=moments, moments_min=moments_min)
    estimate = lambda c, a, n, v: spatial_var_ref(c, a, n, v)
    denoise = lambda c, a, n, v: denoise_var_ref(1, c, a, n, v)[0]
    tables = {}
    for seq in ("static", "moving"):
        refs, frames = [], {spp: [] for spp in spps}
        for f in range(1, FRAMES + 1):
            if seq == "moving" or f == 1:
                arrays = dict(cornell.arrays)
                arrays["transforms"], arrays["inv_transforms"] = moved_consistent(cornell.arrays, f if seq == "moving" else 0)
                osc = ob.OracleScene(arrays, ob.MATH_PORTABLE)
                ref = osc.render(cornell_params(cornell, w, h, ref_spp, cam, 1, 7), want_aovs=False)[0]
                g = gbuffer_cpu(osc, arrays, w, h, cam)
            refs.append(ref)
            for spp in spps:
                c, a, n, _ = osc.render(cornell_params(cornell, w, h, spp, cam, f, 1))
                frames[spp].append({"camera": cam, "transforms": arrays["transforms"], "inv_transforms": arrays["inv_transforms"], "gbuffer": g, "color": c,
                                    "albedo": a, "normal": n, "variance": np.full((h, w), 1e30, np.float32)})
            if seq == "moving" or f == FRAMES:
                osc.close()
            log("%s: frame %d rendered" % (seq, f))
        for spp in spps:
            tables[(seq, spp)] = quality_chain(frames[spp], refs, accumulate, estimate, denoise)
    return tables


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="96x64")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--spps", default="1,4,8")
    ap.add_argument("--moments-min", type=float, default=None, help="history length of the switch (default: the library's HJR_TEMPORAL_MOMENTS_MIN)")
    a = ap.parse_args()
    w, h = map(int, a.size.split("x"))
    print("CPU oracle, NEE, %d x %d, seed 1, camera at x = 3.5, frames 1..%d; references %d spp of seed 7; moments from h >= %s" %
          (w, h, FRAMES, a.ref_spp, "4 (HJR_TEMPORAL_MOMENTS_MIN)" if a.moments_min is None else a.moments_min), flush=True)
    tables = rehearse(Cornell(), w, h, a.ref_spp, tuple(int(s) for s in a.spps.split(",")), a.moments_min, log=lambda s: print(s, flush=True))
    print(format_tables(tables))
    ok = True
    for text, holds in quality_conditions(tables):
        print("%s: %s" % (text, "holds" if holds else "FAILS"))
        ok = ok and holds
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
