#!/usr/bin/env python3
"""tools/temporal_moments_bench.py [--out profiles/temporal_moments.json] [--repeats 5]
What the temporal luminance moments (hjr_temporal_accumulate_moments, option "denoise_temporal_moments") cost and buy.
Run on the GPU machine from the repository root.

  kernel   1920 x 1080, the C2 scene: hjr_temporal_accumulate_moments_device without and with out_moments (hjr_temporal_kernel<false, false>
           and <false, true>), previous = current frame's data with a history of 5 everywhere, so every hit pixel takes the full four-tap
           path and the moments' variance; HIP events around each call on the stream it runs on, the two calls alternating in one loop,
           median of the repeats after one warm-up call each.  Next to it the traffic the moments add at the least: one float2 store per
           pixel and one float2 load per pixel (neighbouring pixels' taps overlap, so each previous value is fetched from memory once).
  frame    hjr_render_denoised, Render_mode Denoise, 1920 x 1080 x 4 spp NEE of the same scene with "denoise_temporal" and
           "denoise_variance_spatial", host wall time of the synchronous call (render + filter + download): two contexts in one process, one
           with "denoise_temporal_moments", rendering the same frames in turn (each keeps its own history); median of the repeats after a
           warm-up frame each.
  quality  the tables of tests/test_gpu_temporal_moments.py::test_quality (96 x 64, frames 1..8, static and moving, 1, 4 and 8 spp; frames
           from the GPU, every stage a CPU checker) with their conditions."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from denoise_var_bench import load  # noqa: E402
from denoise_var_util import denoise_var_ref  # noqa: E402
from scene_util import Cornell, hjr  # noqa: E402
from spatial_var_util import spatial_var_ref  # noqa: E402
from temporal_moments_util import format_tables, quality_chain, quality_conditions, temporal_moments_ref  # noqa: E402
from temporal_util import camera_at, moved_consistent  # noqa: E402

W, H, SPP = 1920, 1080, 4
QW, QH, REF_SPP, QFRAMES = 96, 64, 4096, 8


def quality_tables():
    import numpy as np
    cornell = Cornell()
    dev = cornell.device()
    cam = camera_at(cornell, x=3.5)
    kw = dict(sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)
    nt = np.asarray(cornell.arrays["indices"]).size // 3
    tables = {}
    for seq in ("static", "moving"):
        refs, frames = [], {1: [], 4: [], 8: []}
        for f in range(1, QFRAMES + 1):
            xf = moved_consistent(cornell.arrays, f if seq == "moving" else 0)
            if seq == "moving" or f == 1:
                dev.set_transforms(*xf)
                ref = dev.render(hjr.make_params(QW, QH, REF_SPP, cam, seed=7, **kw), want_aovs=False)[0]
                g = dev.gbuffer(hjr.make_params(QW, QH, 1, cam))
            refs.append(ref)
            for spp in frames:
                c, a, n, v = dev.render(hjr.make_params(QW, QH, spp, cam, frame=f, seed=1, **kw), want_variance=True)
                frames[spp].append({"camera": cam, "transforms": xf[0], "inv_transforms": xf[1], "gbuffer": g, "color": c, "albedo": a, "normal": n, "variance": v})
        for spp in frames:
            tables[(seq, spp)] = quality_chain(frames[spp], refs, lambda prev, cur, moments: temporal_moments_ref(prev, cur, nt, moments=moments),
                                               lambda c, a, n, v: spatial_var_ref(c, a, n, v), lambda c, a, n, v: denoise_var_ref(1, c, a, n, v)[0])
    dev.close()
    return tables


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_moments.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    opt, scene, cam, dev = load("render_option_c2.json")
    L = hjr.lib()
    side = torch.cuda.Stream()
    stream = side.cuda_stream
    assert stream
    kw = dict(seed=opt.seed, integrator=hjr.INTEGRATOR_NEE, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)
    p = hjr.make_params(W, H, SPP, cam, frame=1, **kw)
    col, alb, nrm, acc = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    var, acc_var, acc_hist = (torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(3))
    hist = torch.full((H, W), 5.0, dtype=torch.float32, device="cuda")
    mom = torch.rand((H, W, 2), dtype=torch.float32, device="cuda")
    acc_mom = torch.empty((H, W, 2), dtype=torch.float32, device="cuda")
    gbuf = torch.empty((H, W, hjr.GBUFFER_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    m, inv = scene.transforms(1 / float(opt.fps))
    d_m, d_inv = torch.from_numpy(m).cuda(), torch.from_numpy(inv).cuda()
    dev.render_device(p, col.data_ptr(), alb.data_ptr(), nrm.data_ptr(), stream=stream, d_variance=var.data_ptr())
    dev.estimate_variance_device(W, H, col.data_ptr(), alb.data_ptr(), nrm.data_ptr(), var.data_ptr(), var.data_ptr(), stream=stream)
    assert L.hjr_render_gbuffer_device(dev._h, C.byref(p), gbuf.data_ptr(), stream) == 0, L.hjr_last_error()
    torch.cuda.synchronize()
    fr = hjr.TemporalFrame()
    fr.width, fr.height, fr.n_instances, fr.camera = W, H, m.shape[0], cam
    fr.transforms12, fr.inv_transforms12, fr.gbuffer = d_m.data_ptr(), d_inv.data_ptr(), gbuf.data_ptr()
    fr.color, fr.variance, fr.history = col.data_ptr(), var.data_ptr(), hist.data_ptr()

    def accumulate(out_moments):
        def run():
            rc = L.hjr_temporal_accumulate_moments_device(dev._h, C.byref(fr), C.byref(fr), acc.data_ptr(), acc_var.data_ptr(), acc_hist.data_ptr(), mom.data_ptr(), out_moments, stream)
            assert rc == 0, L.hjr_last_error()
        return run
    kernel_ms = {"accumulate": [], "accumulate_moments": []}
    for r in range(a.repeats + 1):
        for name, fn in (("accumulate", accumulate(None)), ("accumulate_moments", accumulate(acc_mom.data_ptr()))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            fn()
            e1.record(side)
            torch.cuda.synchronize()
            if r:
                kernel_ms[name].append(e0.elapsed_time(e1))
    found = float((acc_hist > 1).float().mean().item())
    switched = float((acc_hist >= 4).float().mean().item())

    # ---- a Denoise frame at 4 spp with and without the option: two contexts, the same frames in turn
    _, _, _, dev_on = load("render_option_c2.json")
    for d, on in ((dev, 0), (dev_on, 1)):
        d.set_option("denoise_temporal", 1)
        d.set_option("denoise_variance_spatial", 1)
        d.set_option("denoise_temporal_moments", on)
    frame_ms = {"temporal_spatial": [], "temporal_spatial_moments": []}
    for r in range(a.repeats + 1):
        q = hjr.make_params(W, H, SPP, cam, frame=1 + r, **kw)
        for name, d in (("temporal_spatial", dev), ("temporal_spatial_moments", dev_on)):
            t0 = time.perf_counter()
            d.render_denoised(q, hjr.MODE_DENOISE)
            if r:
                frame_ms[name].append(1e3 * (time.perf_counter() - t0))
    dev.close()
    dev_on.close()

    tables = quality_tables()
    print(format_tables(tables))
    conditions = [{"text": t, "holds": bool(ok)} for t, ok in quality_conditions(tables)]
    npx = W * H
    res = {
        "what": "temporal luminance moments; MI355X; medians of %d, calls without and with moments alternating in one process" % a.repeats,
        "kernel_1080p_ms": {k: {"median": statistics.median(v), "all": v} for k, v in kernel_ms.items()},
        "kernel_1080p_pixels_with_history": found,
        "kernel_1080p_pixels_past_the_switch": switched,
        "moments_minimum_extra_traffic_bytes": {"load_float2_per_pixel": npx * 8, "store_float2_per_pixel": npx * 8, "total": npx * 16},
        "denoise_frame_1080p_4spp_wall_ms": {k: {"median": statistics.median(v), "all": v} for k, v in frame_ms.items()},
        "quality_96x64_nee_ref_4096spp": {"%s_%dspp" % k: v for k, v in sorted(tables.items())},
        "quality_conditions": conditions,
    }
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if not k.startswith("quality_96")}, indent=1))
    return 0 if all(c["holds"] for c in conditions) else 1


if __name__ == "__main__":
    sys.exit(main())
