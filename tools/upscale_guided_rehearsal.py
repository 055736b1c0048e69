#!/usr/bin/env python3
"""tools/upscale_guided_rehearsal.py [--size 96x64] [--spp 64] [--ref-spp 4096] [--k-plane 1 --k-normal 0.9]
CPU rehearsal of the quality comparison of tests/test_gpu_upscale_guided.py: no GPU, every stage from a CPU restatement.

  frames     the CPU oracle (oracle/), NEE, seed 1, rendered at half of --size with --spp samples; the variance AOV by rule 7 from the
             oracle's per-sample radiance; camera at x = 3.5 (asserted) and the scene's own camera (reported)
  G-buffers  tools/temporal_rehearsal.gbuffer_cpu (the oracle's brute-force closest hit of the pixel-centre rays) at both sizes
  stages     tests/native/denoise_var_ref.cpp (variance-guided filter, Denoise mode), tests/native/upscale_guided_ref.cpp (guided upscale),
             the numpy restatement of the bilinear upscale
  reference  the oracle rendered directly at --size with --ref-spp samples, seed 7
Prints the table and the condition of the GPU test; exit status 1 if it fails."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_binding as ob  # noqa: E402
from denoise_var_util import denoise_var_ref, variance_rule  # noqa: E402
from scene_util import Cornell, hjr  # noqa: E402
from temporal_rehearsal import cornell_params, gbuffer_cpu  # noqa: E402
from upscale_guided_util import Q_SPP, QH, QW, REF_SPP, bilinear_np, format_table, quality_conditions, quality_row, upscale_guided_ref  # noqa: E402

f32 = np.float32


def frame_with_variance(osc, op, w, h, spp):
    """colour, albedo, normal of the oracle's frame and the variance AOV (rule 7) from its per-sample radiance."""
    c, a, n, _ = osc.render(op)
    g = hjr.sample_granule(spp)
    chunks = np.zeros((spp // g, h, w, 3), f32)
    for y in range(h):
        for x in range(w):
            for s in range(spp):
                chunks[s // g, y, x] = chunks[s // g, y, x] + osc.sample(op, x, y, s)[0]
    return c, a, n, variance_rule(chunks, g, spp // g, spp)


def rehearse(cornell, ow, oh, spp, ref_spp, k=None, cameras=("x = 3.5", "scene camera"), log=None):
    """{camera name: quality_row} of the CPU oracle's frames."""
    log = log or (lambda s: None)
    iw, ih = ow // 2, oh // 2
    osc = ob.OracleScene(cornell.arrays, ob.MATH_PORTABLE)
    table = {}
    for name in cameras:
        cam = hjr.Camera.from_buffer_copy(cornell.camera)
        if name == "x = 3.5":
            cam.pos[0] = 3.5
        cam = cam.as_dict()
        ref = osc.render(cornell_params(cornell, ow, oh, ref_spp, cam, 1, 7), want_aovs=False)[0]
        log("%s: reference rendered" % name)
        c, a, n, v = frame_with_variance(osc, cornell_params(cornell, iw, ih, spp, cam, 1, 1), iw, ih, spp)
        filtered = denoise_var_ref(1, c, a, n, v)[0]
        log("%s: frame rendered and filtered" % name)
        g_lo, g_hi = gbuffer_cpu(osc, cornell.arrays, iw, ih, cam), gbuffer_cpu(osc, cornell.arrays, ow, oh, cam)
        guided, count = upscale_guided_ref(filtered, g_lo, cam, g_hi, k)
        table[name] = dict(quality_row(guided, bilinear_np(filtered, ow, oh), ref), partial_share=float(((count > 0) & (count < 4)).mean()))
    osc.close()
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="%dx%d" % (QW, QH))
    ap.add_argument("--spp", type=int, default=Q_SPP)
    ap.add_argument("--ref-spp", type=int, default=REF_SPP)
    ap.add_argument("--k-plane", type=float, default=None)
    ap.add_argument("--k-normal", type=float, default=None)
    a = ap.parse_args()
    w, h = map(int, a.size.split("x"))
    k = None if a.k_plane is None and a.k_normal is None else (1.0 if a.k_plane is None else a.k_plane, 0.9 if a.k_normal is None else a.k_normal)
    table = rehearse(Cornell(), w, h, a.spp, a.ref_spp, k, log=lambda s: print(s, flush=True))
    print(format_table(table))
    for name, r in table.items():
        print("%s: %.1f %% of the pixels have 1 to 3 valid taps" % (name, 100 * r["partial_share"]))
    ok = True
    for text, holds in quality_conditions(table):
        print("%s: %s" % (text, "holds" if holds else "FAILS"))
        ok = ok and holds
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
