#!/usr/bin/env python3
"""tools/temporal_response_bench.py [--out profiles/temporal_response.json] [--repeats 5]
What the windowed change test of the temporal accumulation (hjr_temporal_accumulate_response, option "denoise_temporal_response",
DESIGN.md §11.8) costs.  Run on the GPU machine from the repository root.

  kernel   1920 x 1080, the C2 scene: hjr_temporal_accumulate_response_device without and with out_response (hjr_temporal_kernel<false, MOM>
           and hjr_temporal_resp_kernel<false, MOM>), without and with the moments; previous = current frame's data with a history of 5
           everywhere, so every hit pixel takes the full four-tap path and is a member of its neighbours' windows (lambda = 0: the
           arithmetic does not depend on it); HIP events around each call on the stream it runs on, the four calls alternating in one
           loop, median of the repeats after one warm-up call each.  The new kernel gathers 400 cells per 256 pixels (1.56 x the
           reprojections) and reads 75 LDS words per pixel.
  frame    hjr_render_denoised, Render_mode Denoise, 1920 x 1080 x 16 spp NEE of the same scene with "denoise_temporal", host wall time of the
           synchronous call (render + filter + download): two contexts in one process, one with "denoise_temporal_response", rendering the
           same frames in turn (each keeps its own history); median of the repeats after a warm-up frame each."""
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
from scene_util import hjr  # noqa: E402

W, H, SPP = 1920, 1080, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_response.json"))
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
    var, acc_var, acc_hist, acc_lam = (torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(4))
    hist = torch.full((H, W), 5.0, dtype=torch.float32, device="cuda")
    mom = torch.rand((H, W, 2), dtype=torch.float32, device="cuda")
    acc_mom = torch.empty((H, W, 2), dtype=torch.float32, device="cuda")
    gbuf = torch.empty((H, W, hjr.GBUFFER_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    m, inv = scene.transforms(1 / float(opt.fps))
    d_m, d_inv = torch.from_numpy(m).cuda(), torch.from_numpy(inv).cuda()
    dev.render_device(p, col.data_ptr(), alb.data_ptr(), nrm.data_ptr(), stream=stream, d_variance=var.data_ptr())
    assert L.hjr_render_gbuffer_device(dev._h, C.byref(p), gbuf.data_ptr(), stream) == 0, L.hjr_last_error()
    torch.cuda.synchronize()
    fr = hjr.TemporalFrame()
    fr.width, fr.height, fr.n_instances, fr.camera = W, H, m.shape[0], cam
    fr.transforms12, fr.inv_transforms12, fr.gbuffer = d_m.data_ptr(), d_inv.data_ptr(), gbuf.data_ptr()
    fr.color, fr.variance, fr.history = col.data_ptr(), var.data_ptr(), hist.data_ptr()

    def accumulate(out_moments, out_response):
        def run():
            rc = L.hjr_temporal_accumulate_response_device(dev._h, C.byref(fr), C.byref(fr), acc.data_ptr(), acc_var.data_ptr(), acc_hist.data_ptr(), mom.data_ptr(), out_moments,
                                                           out_response, stream)
            assert rc == 0, L.hjr_last_error()
        return run
    calls = (("accumulate", accumulate(None, None)), ("accumulate_response", accumulate(None, acc_lam.data_ptr())),
             ("accumulate_moments", accumulate(acc_mom.data_ptr(), None)), ("accumulate_moments_response", accumulate(acc_mom.data_ptr(), acc_lam.data_ptr())))
    kernel_ms = {name: [] for name, _ in calls}
    for r in range(a.repeats + 1):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            fn()
            e1.record(side)
            torch.cuda.synchronize()
            if r:
                kernel_ms[name].append(e0.elapsed_time(e1))
    found = float((acc_hist > 1).float().mean().item())
    answered = float((acc_lam > 0).float().mean().item())

    # ---- a Denoise frame with and without the option: two contexts, the same frames in turn
    _, _, _, dev_on = load("render_option_c2.json")
    for d, on in ((dev, 0), (dev_on, 1)):
        d.set_option("denoise_temporal", 1)
        d.set_option("denoise_temporal_response", on)
    frame_ms = {"temporal": [], "temporal_response": []}
    for r in range(a.repeats + 1):
        q = hjr.make_params(W, H, SPP, cam, frame=1 + r, **kw)
        for name, d in (("temporal", dev), ("temporal_response", dev_on)):
            t0 = time.perf_counter()
            d.render_denoised(q, hjr.MODE_DENOISE)
            if r:
                frame_ms[name].append(1e3 * (time.perf_counter() - t0))
    dev.close()
    dev_on.close()

    res = {
        "what": "windowed change test of the temporal accumulation; MI355X; medians of %d, the calls alternating in one process" % a.repeats,
        "kernel_1080p_ms": {k: {"median": statistics.median(v), "all": v} for k, v in kernel_ms.items()},
        "kernel_1080p_pixels_with_history": found,
        "kernel_1080p_pixels_with_lambda_above_0": answered,
        "denoise_frame_1080p_16spp_wall_ms": {k: {"median": statistics.median(v), "all": v} for k, v in frame_ms.items()},
    }
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
