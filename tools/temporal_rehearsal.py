#!/usr/bin/env python3
"""tools/temporal_rehearsal.py [--size 48x32] [--ref-spp 4096] [--k-plane 1 --k-dist 3] [--coverage N [--snap 0.125]] [--seed 1] [--sequences SM]
CPU rehearsal of the quality comparison of tests/test_gpu_temporal.py: no GPU, every stage from a CPU restatement.

  frames     the CPU oracle (oracle/), NEE, 16 spp, seed 1, frames 1..8 with `frame` advancing, camera at x = 3.5; the variance AOV by rule 7
             from the oracle's per-sample radiance (chunks of 8 samples); sequence S static, sequence M every instance moved by
             frame * (0.05, -0.03, 0.02)
  G-buffer   the oracle's brute-force closest hit (tests/trace_util.brute_closest) of the pixel-centre rays, pos / ng from the world-space
             triangles in numpy
  stages     tests/native/temporal_ref.cpp (accumulation) and tests/native/denoise_var_ref.cpp (variance-guided filter)
  reference  the oracle at --ref-spp samples, seed 7, of each frame's geometry (one for S, one per frame for M)
  --coverage N (2, 3 or 4) adds a third column, the temporal path with the coverage G-buffer of side N and rules 2' / 3':
             G-buffer and accumulation from tests/native/temporal_cov_ref.cpp (brute force over the world-space triangles in numpy's
             float32), and prints §11.5's conditions; --snap overrides HJR_TEMPORAL_SNAP in the checker (the one re-tune); --seed is the
             seed of the 16 spp frames; --json FILE appends the tables
Prints the table and the conditions; exit status 1 if a condition of sequence S fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_binding as ob  # noqa: E402
import trace_util  # noqa: E402
from denoise_var_util import denoise_var_ref, variance_rule  # noqa: E402
from scene_util import Cornell, hjr  # noqa: E402
import temporal_cov_util as tcu  # noqa: E402
from temporal_util import MISS, centre_rays, format_table, moved_consistent, quality_conditions, quality_table, temporal_ref  # noqa: E402

f32 = np.float32
SPP, FRAMES = 16, 8


def gbuffer_cpu(osc, arrays, w, h, cam):
    d, pos = centre_rays(w, h, cam)
    o = np.broadcast_to(pos, (h * w, 3)).astype(f32)
    prim, tb = trace_util.brute_closest(osc, o, d.reshape(-1, 3))
    tris = trace_util.world_triangles(arrays)
    po = np.asarray(arrays["prim_offsets"]).reshape(-1)
    g = np.zeros(h * w, hjr.GBUFFER_DTYPE)
    g["prim"] = MISS
    hit = prim != trace_util.NO_PRIM
    k = prim[hit].astype(np.int64)
    b1, b2 = tb[hit, 1], tb[hit, 2]
    v0, v1, v2 = tris[k, 0], tris[k, 1], tris[k, 2]
    w0 = (f32(1) - b1) - b2
    g["prim"][hit] = prim[hit]
    g["inst"][hit] = (np.searchsorted(po, k, side="right") - 1).astype(np.uint32)
    g["t"][hit], g["b1"][hit], g["b2"][hit] = tb[hit, 0], b1, b2
    g["pos"][hit] = (v0 * w0[:, None] + v1 * b1[:, None]) + v2 * b2[:, None]
    g["ng"][hit] = np.cross(v1 - v0, v2 - v0).astype(f32)
    return g.reshape(h, w)


def frame_cpu(osc, op, w, h):
    """colour, albedo, normal of the oracle's frame and the variance AOV from its per-sample radiance."""
    c, a, n, _ = osc.render(op)
    g = hjr.sample_granule(SPP)
    chunks = np.zeros((SPP // g, h, w, 3), f32)
    for y in range(h):
        for x in range(w):
            for s in range(SPP):
                chunks[s // g, y, x] = chunks[s // g, y, x] + osc.sample(op, x, y, s)[0]
    return c, a, n, variance_rule(chunks, g, SPP // g, SPP)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="48x32")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--k-plane", type=float, default=1.0)
    ap.add_argument("--k-dist", type=float, default=3.0)
    ap.add_argument("--coverage", type=int, default=0, choices=(0, 2, 3, 4))
    ap.add_argument("--snap", type=float, default=None)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sequences", default="SM")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    w, h = map(int, a.size.split("x"))
    cornell = Cornell()
    cam = hjr.Camera.from_buffer_copy(cornell.camera)
    cam.pos[0] = 3.5
    cam = cam.as_dict()
    n_tris = np.asarray(cornell.arrays["indices"]).size // 3
    ok = True
    tables = {}
    for name, static in (("S", True), ("M", False)):
        if name not in a.sequences:
            continue
        refs, out_var, out_tmp, out_cov = [], [], [], []
        prev = prev_cov = None
        for f in range(1, FRAMES + 1):
            arrays = dict(cornell.arrays)
            if not static:
                arrays["transforms"], arrays["inv_transforms"] = moved_consistent(cornell.arrays, f)
            osc = ob.OracleScene(arrays, ob.MATH_PORTABLE)
            if not static or f == 1:
                ref = osc.render(cornell_params(cornell, w, h, a.ref_spp, cam, 1, 7), want_aovs=False)[0]
            refs.append(ref)
            c, al, n, v = frame_cpu(osc, cornell_params(cornell, w, h, SPP, cam, f, a.seed), w, h)
            cur = {"camera": cam, "transforms": arrays["transforms"], "inv_transforms": arrays["inv_transforms"], "gbuffer": gbuffer_cpu(osc, arrays, w, h, cam),
                   "color": c, "variance": v}
            tc, tv, th = temporal_ref(prev, cur, n_tris, (a.k_plane, a.k_dist))
            out_var.append(denoise_var_ref(1, c, al, n, v)[0])
            out_tmp.append(denoise_var_ref(1, tc, al, n, tv)[0])
            prev = dict(cur, color=tc, variance=tv, history=th)
            if a.coverage:
                g = tcu.gbuffer_cov_ref(*tcu.rows_from_arrays(arrays), w, h, cam, a.coverage)
                cur = dict(cur, gbuffer=g, coverage=a.coverage)
                cc, cv, ch = tcu.temporal_cov_ref(prev_cov, cur, n_tris, a.snap)
                out_cov.append(denoise_var_ref(1, cc, al, n, cv)[0])
                prev_cov = dict(cur, color=cc, variance=cv, history=ch)
                print("%s frame %d, coverage %d: %d mixed pixels, mean history %.2f, restarted %.1f %%" % (name, f, a.coverage, int(tcu.mixed(g).sum()), float(ch.mean()),
                                                                                                      100 * float((ch == 1).mean())), flush=True)
            print("%s frame %d: mean history %.2f, restarted %.1f %%" % (name, f, float(th.mean()), 100 * float((th == 1).mean())), flush=True)
            osc.close()
        if a.coverage:
            t = tcu.quality_table_cov(refs, out_var, out_tmp, out_cov)
            print(tcu.format_table_cov(name, t))
            for text, holds in tcu.conditions_s(t) if static else tcu.conditions_m(t):
                print("%s   %s: %s" % (name, text, "holds" if holds else "FAILS"))
        else:
            t = quality_table(refs, out_var, out_tmp)
            print(format_table(name, t))
        tables[name] = t
        for text, holds in quality_conditions(t, static):
            print("%s   %s: %s" % (name, text, "holds" if holds else "FAILS"))
            ok = ok and (holds or not static)
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps({"size": a.size, "seed": a.seed, "coverage": a.coverage, "snap": a.snap, "ref_spp": a.ref_spp, "tables": tables}) + "\n")
    return 0 if ok else 1


def cornell_params(cornell, w, h, spp, cam, frame, seed):
    return ob.make_params(w, h, spp, cam, frame=frame, seed=seed, sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)


if __name__ == "__main__":
    sys.exit(main())
