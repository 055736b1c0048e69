#!/usr/bin/env python3
"""tools/spatial_var_rehearsal.py [--size 96x64] [--ref-spp 4096] [--radius 1] [--no-chains]
CPU rehearsal of the quality comparison of tests/test_gpu_spatial_var.py: no GPU, every stage from a CPU restatement.

  frames     the CPU oracle (oracle/), NEE, seed 1, camera at x = 3.5; 1, 2, 4 and 8 spp, frames 1..4 (single frames) and 4 spp, frames 1..8
             with `frame` advancing (temporal chains; static, and every instance moved by frame * (0.05, -0.03, 0.02)).  Every such frame is
             a single chunk, so its variance AOV is HJR_VARIANCE_UNKNOWN everywhere
  G-buffer   tools/temporal_rehearsal.gbuffer_cpu (the oracle's brute-force closest hit of the pixel-centre rays)
  stages     tests/native/spatial_var_ref.cpp (the estimate), tests/native/temporal_ref.cpp (accumulation), tests/native/denoise_var_ref.cpp
             (variance-guided filter), the oracle's plain filter
  reference  the oracle at --ref-spp samples, seed 7, of each frame's geometry
Prints both tables and the conditions of the GPU test; exit status 1 if one fails."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_binding as ob  # noqa: E402
from scene_util import Cornell, hjr  # noqa: E402
from spatial_var_util import (CHAIN_FRAMES, CHAIN_SPP, beats_plain_share, format_tables, quality_conditions, single_frame_table,  # noqa: E402
                              temporal_chain)
from temporal_rehearsal import cornell_params, gbuffer_cpu  # noqa: E402
from temporal_util import moved_consistent  # noqa: E402


def rehearse(cornell, w, h, ref_spp, radius=None, chains=True, spps=None, log=None):
    """(single-frame table, {"static": chain, "moving": chain} or {}) of the CPU oracle's frames."""
    cam = hjr.Camera.from_buffer_copy(cornell.camera)
    cam.pos[0] = 3.5
    cam = cam.as_dict()
    n_tris = np.asarray(cornell.arrays["indices"]).size // 3
    log = log or (lambda s: None)

    def scene(k):
        arrays = dict(cornell.arrays)
        if k:
            arrays["transforms"], arrays["inv_transforms"] = moved_consistent(cornell.arrays, k)
        return arrays, ob.OracleScene(arrays, ob.MATH_PORTABLE)

    arrays0, osc0 = scene(0)
    ref0 = osc0.render(cornell_params(cornell, w, h, ref_spp, cam, 1, 7), want_aovs=False)[0]
    log("reference of the static geometry rendered")
    kw = {} if spps is None else {"spps": spps}
    table = single_frame_table(lambda spp, f: osc0.render(cornell_params(cornell, w, h, spp, cam, f, 1))[:3], ref0, radius=radius, **kw)
    out = {}
    if chains:
        g0 = gbuffer_cpu(osc0, arrays0, w, h, cam)
        for name in ("static", "moving"):
            refs, frames = [], {}
            for f in range(1, CHAIN_FRAMES + 1):
                arrays, osc = (arrays0, osc0) if name == "static" else scene(f)
                refs.append(ref0 if name == "static" else osc.render(cornell_params(cornell, w, h, ref_spp, cam, 1, 7), want_aovs=False)[0])
                c, a, n, _ = osc.render(cornell_params(cornell, w, h, CHAIN_SPP, cam, f, 1))
                side = {"camera": cam, "transforms": arrays["transforms"], "inv_transforms": arrays["inv_transforms"],
                        "gbuffer": g0 if name == "static" else gbuffer_cpu(osc, arrays, w, h, cam)}
                frames[f] = (c, a, n, side)
                if osc is not osc0:
                    osc.close()
                log("%s chain: frame %d rendered" % (name, f))
            out[name] = temporal_chain(lambda f: frames[f], refs, n_tris, radius=radius)
    osc0.close()
    return table, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="96x64")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--radius", type=int, default=1, help="window radius of the estimate (1 = the library's 3 x 3)")
    ap.add_argument("--no-chains", action="store_true")
    a = ap.parse_args()
    w, h = map(int, a.size.split("x"))
    table, chains = rehearse(Cornell(), w, h, a.ref_spp, radius=a.radius, chains=not a.no_chains, log=lambda s: print(s, flush=True))
    print(format_tables(table, chains))
    ok = True
    for text, holds in quality_conditions(table, chains):
        print("%s: %s" % (text, "holds" if holds else "FAILS"))
        ok = ok and holds
    if chains:
        print("frames 2..%d of the chains below the plain filter: %.0f %% (reported, not asserted)" % (CHAIN_FRAMES, 100 * beats_plain_share(chains)))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
