#!/usr/bin/env python3
"""tools/temporal_bench.py [--out profiles/temporal.json] [--out-coverage profiles/temporal_coverage.json] [--repeats 5]
What temporal accumulation with reprojection (hjr_render_gbuffer / hjr_temporal_accumulate, option "denoise_temporal")
costs and buys.  Run on the GPU machine from the repository root.

  kernels  1920 x 1080, the C2 scene: hjr_render_gbuffer_device and hjr_temporal_accumulate_device (previous = current frame's data, so
           every hit pixel takes the full four-tap path), HIP events around each call on the stream it runs on, median of the repeats
           after one warm-up call each; next to them, alternating in the same loop, the coverage pass (hjr_render_gbuffer_cov_device) at
           side 2 and side 4 and the accumulation with `coverage` set on both sides.
  frame    hjr_render_denoised, Render_mode Denoise, 1920 x 1080 x 16 spp NEE of the same scene, host wall time of the synchronous call
           (render + filter + download), median of the repeats after a warm-up: option "denoise_temporal" 1 against the same build with
           "denoise_variance" 1 alone and with neither, and with "denoise_temporal_coverage" 4 on top.
  quality  the table of tests/test_gpu_temporal.py::test_quality_temporal_path_beats_the_per_frame_filter (96 x 64, 16 spp per frame,
           frames 1..8, static and moving sequence) and of tests/test_gpu_temporal_cov.py::test_quality_tables (the same renders with the
           coverage column), the latter written to --out-coverage with the coverage kernels' timings.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from denoise_var_bench import load  # noqa: E402
from scene_util import Cornell, hjr  # noqa: E402
from temporal_cov_util import conditions_m, conditions_s, format_table_cov, quality_sequences_cov  # noqa: E402
from temporal_util import format_table, quality_conditions  # noqa: E402

W, H, SPP = 1920, 1080, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal.json"))
    ap.add_argument("--out-coverage", default=os.path.join(ROOT, "profiles", "temporal_coverage.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    opt, scene, cam, dev = load("render_option_c2.json")
    L = hjr.lib()
    side = torch.cuda.Stream()
    stream = side.cuda_stream
    assert stream
    kw = dict(frame=1, seed=opt.seed, integrator=hjr.INTEGRATOR_NEE, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)
    p = hjr.make_params(W, H, SPP, cam, **kw)
    col, alb, nrm, acc = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    var, acc_var, acc_hist = (torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(3))
    hist = torch.full((H, W), 5.0, dtype=torch.float32, device="cuda")
    gbuf = torch.empty((H, W, hjr.GBUFFER_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    gbuf_cov = torch.empty((H, W, hjr.GBUFFER_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    m, inv = scene.transforms(1 / float(opt.fps))
    d_m, d_inv = torch.from_numpy(m).cuda(), torch.from_numpy(inv).cuda()
    dev.render_device(p, col.data_ptr(), alb.data_ptr(), nrm.data_ptr(), stream=stream, d_variance=var.data_ptr())
    torch.cuda.synchronize()

    fr = hjr.TemporalFrame()
    fr.width, fr.height, fr.n_instances, fr.camera = W, H, m.shape[0], cam
    fr.transforms12, fr.inv_transforms12, fr.gbuffer = d_m.data_ptr(), d_inv.data_ptr(), gbuf.data_ptr()
    fr.color, fr.variance, fr.history = col.data_ptr(), var.data_ptr(), hist.data_ptr()

    fr_cov = hjr.TemporalFrame.from_buffer_copy(fr)
    fr_cov.gbuffer, fr_cov.coverage = gbuf_cov.data_ptr(), 4

    def gbuffer_cov(n):
        def run():
            rc = L.hjr_render_gbuffer_cov_device(dev._h, C.byref(p), n, gbuf_cov.data_ptr(), stream)
            assert rc == 0, L.hjr_last_error()
        return run

    def accumulate_cov():
        rc = L.hjr_temporal_accumulate_device(dev._h, C.byref(fr_cov), C.byref(fr_cov), acc.data_ptr(), acc_var.data_ptr(), acc_hist.data_ptr(), stream)
        assert rc == 0, L.hjr_last_error()

    def gbuffer():
        rc = L.hjr_render_gbuffer_device(dev._h, C.byref(p), gbuf.data_ptr(), stream)
        assert rc == 0, L.hjr_last_error()

    def accumulate():
        rc = L.hjr_temporal_accumulate_device(dev._h, C.byref(fr), C.byref(fr), acc.data_ptr(), acc_var.data_ptr(), acc_hist.data_ptr(), stream)
        assert rc == 0, L.hjr_last_error()
    kernel_ms = {"gbuffer": [], "accumulate": [], "gbuffer_cov_side2": [], "gbuffer_cov_side4": [], "accumulate_cov": []}
    for r in range(a.repeats + 1):  # option off and option on alternate; accumulate_cov reads the side-4 records written just before it
        for name, fn in (("gbuffer", gbuffer), ("gbuffer_cov_side2", gbuffer_cov(2)), ("accumulate", accumulate), ("gbuffer_cov_side4", gbuffer_cov(4)),
                         ("accumulate_cov", accumulate_cov)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            fn()
            e1.record(side)
            torch.cuda.synchronize()
            if r:
                kernel_ms[name].append(e0.elapsed_time(e1))
    found_cov = float((acc_hist > 1).float().mean().item())
    accumulate()
    torch.cuda.synchronize()
    found = float((acc_hist > 1).float().mean().item())
    pad = gbuf_cov.cpu().numpy().reshape(-1).view(hjr.GBUFFER_DTYPE)["pad"]
    mixed_share = float(((pad & 0xff) < ((pad >> 8) & 0xff)).mean())

    # ---- a Denoise frame with and without the option (host wall time of the synchronous call)
    frame_ms = {"plain_filter": [], "denoise_variance": [], "denoise_temporal": [], "denoise_temporal_coverage4": []}
    for name, options in (("plain_filter", {}), ("denoise_variance", {"denoise_variance": 1}), ("denoise_temporal", {"denoise_temporal": 1}),
                          ("denoise_temporal_coverage4", {"denoise_temporal": 1, "denoise_temporal_coverage": 4})):
        for k in ("denoise_variance", "denoise_temporal", "denoise_temporal_coverage"):
            dev.set_option(k, options.get(k, 0))
        for r in range(a.repeats + 1):
            q = hjr.make_params(W, H, SPP, cam, **dict(kw, frame=1 + r))
            t0 = time.perf_counter()
            dev.render_denoised(q, hjr.MODE_DENOISE)
            if r:
                frame_ms[name].append(1e3 * (time.perf_counter() - t0))
    dev.close()

    # ---- quality (the test's sequences)
    cornell = Cornell()
    d = cornell.device()
    cov_tables = quality_sequences_cov(cornell, d, 4)  # (the e_var and e_tmp columns are quality_sequences': the same renders and calls)
    d.close()
    tables = {}
    for name in ("S", "M"):
        print(format_table_cov(name, cov_tables[name]))
        tables[name] = {k: v for k, v in cov_tables[name].items() if not k.endswith("_cov")}
        print(format_table(name, tables[name]))
        tables[name]["conditions"] = [{"text": t, "holds": bool(ok)} for t, ok in quality_conditions(tables[name], name == "S")]
        cov_tables[name]["conditions"] = [{"text": t, "holds": bool(ok)} for t, ok in (conditions_s if name == "S" else conditions_m)(cov_tables[name])]

    res = {
        "what": "temporal accumulation with reprojection; MI355X; medians of %d" % a.repeats,
        "kernels_1080p_ms": {k: {"median": statistics.median(v), "all": v} for k, v in kernel_ms.items() if "cov" not in k},
        "accumulate_pixels_with_history": found,
        "denoise_frame_1080p_16spp_wall_ms": {k: {"median": statistics.median(v), "all": v} for k, v in frame_ms.items()},
        "quality_96x64_nee_16spp_ref_4096spp": tables,
    }
    cov = {
        "what": "coverage-aware temporal accumulation (side 4 unless said otherwise); MI355X; medians of %d, plain and coverage calls alternating in one process" % a.repeats,
        "kernels_1080p_ms": {k: {"median": statistics.median(v), "all": v} for k, v in kernel_ms.items()},
        "mixed_pixels_1080p_share": mixed_share,
        "accumulate_cov_pixels_with_history": found_cov,
        "denoise_frame_1080p_16spp_wall_ms": {k: {"median": statistics.median(v), "all": v} for k, v in frame_ms.items() if "temporal" in k},
        "quality_96x64_nee_16spp_ref_4096spp_side4": cov_tables,
    }
    for path, obj in ((a.out, res), (a.out_coverage, cov)):
        with open(path, "w") as f:
            json.dump(obj, f, indent=1)
            f.write("\n")
        print(json.dumps(obj, indent=1))


if __name__ == "__main__":
    main()
