#!/usr/bin/env python3
"""tools/temporal_response_rehearsal.py [--size 96x64] [--ref-spp 4096] [--sequences SLM] [--radius 2]
CPU rehearsal of the quality comparison of tests/test_gpu_temporal_response.py: no GPU, every stage from a CPU restatement.

  frames     the CPU oracle (oracle/), NEE, 16 spp, seed 1, camera at x = 3.5; frames 1..10 with `frame` advancing; the variance AOV by
             rule 7 from the oracle's per-sample radiance (tools/temporal_rehearsal.frame_cpu).  Sequence S is static, M moves every
             instance by frame * (0.05, -0.03, 0.02), and L moves only the instance that holds the light, by (0.12 * max(0, frame - 3), 0, 0)
  G-buffer   tools/temporal_rehearsal.gbuffer_cpu (the oracle's brute-force closest hit of the pixel-centre rays)
  stages     tests/native/temporal_response_ref.cpp (accumulation, without and with the change test), tests/native/denoise_var_ref.cpp
  reference  the oracle at --ref-spp samples, seed 7, of each frame's geometry; the mask of §11.2
Three columns per sequence: the per-frame variance-guided filter, the temporal path, the temporal path with the change test.  Prints the
tables, the ten worst pixels of M's worst frame and the conditions of the GPU test (on S and L; it runs the sizes 96x64 with 4096 spp
references and 48x32 with 2048); exit status 1 if an asserted one fails."""
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
from temporal_rehearsal import cornell_params, frame_cpu, gbuffer_cpu  # noqa: E402
from temporal_response_util import (QFRAMES, format_tables, geometry_changes, quality_chain, quality_conditions, sequence_transforms,  # noqa: E402
                                    temporal_response_ref, worst_pixels)
from temporal_util import ref_mask  # noqa: E402


def rehearse(cornell, w, h, ref_spp, sequences="SLM", radius=None, frames=QFRAMES, log=None):
    """{sequence: table} of the CPU oracle's frames (tests/temporal_response_util.quality_chain) and {sequence: references}."""
    cam = hjr.Camera.from_buffer_copy(cornell.camera)
    cam.pos[0] = 3.5
    cam = cam.as_dict()
    n_tris = np.asarray(cornell.arrays["indices"]).size // 3
    log = log or (lambda s: None)
    accumulate = lambda prev, cur, response: temporal_response_ref(prev, cur, n_tris, response=response, radius=radius)
    denoise = lambda c, a, n, v: denoise_var_ref(1, c, a, n, v)[0]
    tables, all_refs = {}, {}
    for seq in sequences:
        refs, rendered = [], []
        for f in range(1, frames + 1):
            arrays = dict(cornell.arrays)
            arrays["transforms"], arrays["inv_transforms"] = sequence_transforms(cornell.arrays, seq, f)
            osc = ob.OracleScene(arrays, ob.MATH_PORTABLE)
            if geometry_changes(seq, f):
                ref = osc.render(cornell_params(cornell, w, h, ref_spp, cam, 1, 7), want_aovs=False)[0]
                g = gbuffer_cpu(osc, arrays, w, h, cam)
            refs.append(ref)
            c, a, n, v = frame_cpu(osc, cornell_params(cornell, w, h, 16, cam, f, 1), w, h)
            rendered.append({"camera": cam, "transforms": arrays["transforms"], "inv_transforms": arrays["inv_transforms"], "gbuffer": g, "color": c,
                             "albedo": a, "normal": n, "variance": v})
            osc.close()
            log("%s: frame %d rendered" % (seq, f))
        tables[seq] = quality_chain(rendered, refs, accumulate, denoise)
        all_refs[seq] = refs
    return tables, all_refs


def report_worst(t, refs):
    """The ten worst pixels of the worst e_resp frame of a table."""
    f = int(np.argmax(t["e_resp"]))
    return ["worst frame %d (e_resp %.5f, e_tmp %.5f)" % (f + 1, t["e_resp"][f], t["e_tmp"][f])] + worst_pixels(t["out_resp"][f], refs[f], ref_mask(refs[f]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="96x64")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--sequences", default="SLM")
    ap.add_argument("--radius", type=int, default=None, help="window radius (default: the library's HJR_TEMPORAL_RESP_R = 2)")
    a = ap.parse_args()
    w, h = map(int, a.size.split("x"))
    print("CPU oracle, NEE, %d x %d, 16 spp, seed 1, camera at x = 3.5, frames 1..%d; references %d spp of seed 7; window radius %s" %
          (w, h, QFRAMES, a.ref_spp, "2 (HJR_TEMPORAL_RESP_R)" if a.radius is None else a.radius), flush=True)
    tables, refs = rehearse(Cornell(), w, h, a.ref_spp, a.sequences, a.radius, log=lambda s: print(s, flush=True))
    print(format_tables(tables))
    if "M" in tables:
        print("\n".join("M   " + s for s in report_worst(tables["M"], refs["M"])))
    ok = True
    for text, holds, asserted in quality_conditions(tables, (w, h)):
        print("%s: %s" % (text, "holds" if holds else "FAILS" if asserted else "fails (reported at this size, not asserted)"))
        ok = ok and (holds or not asserted)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
