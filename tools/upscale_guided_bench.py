#!/usr/bin/env python3
"""tools/upscale_guided_bench.py [--out profiles/upscale_guided.json] [--repeats 5] [--no-quality] [--trace-run]
What the guided 2x upscale (hjr_upscale_guided, option "upscale_guided") costs and buys.  Run on the GPU machine from the
repository root.

  cost     DenoiseUpScale2X at 1920 x 1080 output: 960 x 540 x 256 spp, NEE, the bundled scene, "denoise_variance" on.
           frame    hjr_render_denoised, option off against on, alternating in this process: wall clock of the synchronous call (render,
                    post stage and the copy of the 1080p image to the host), median of the repeats after one warm-up round.
           stages   the same frame's AOVs on the device, each stage through its device-form call on one stream with HIP events around
                    it, alternating, median of the repeats: the five filter passes (hjr_denoise_var_device, Denoise mode), the five passes
                    plus the bilinear upscale (the 2x mode: the parent's post stage), the G-buffer at 960 x 540 and at 1920 x 1080, the
                    guided kernel, and the whole guided post stage (filter, both G-buffers, kernel) in one window.
  quality  the table of tools/upscale_guided_rehearsal.py from GPU frames (96 x 64 output, 48 x 32 x 64 spp, reference 4096 spp at 96 x 64),
           every stage a library call; reported with its condition, which the CPU rehearsal already saw fail from the camera at x = 3.5.
  --trace-run   three frames with the option on and nothing else: the run to put under a kernel trace for the dispatch times.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from scene_util import Cornell, hjr  # noqa: E402
from upscale_guided_util import format_table, gpu_quality_table, quality_conditions  # noqa: E402

OW, OH, SPP = 1920, 1080, 256
W, H = OW // 2, OH // 2
UP = hjr.MODE_DENOISE_UPSCALE2X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upscale_guided.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    import torch
    cornell = Cornell()
    dev = cornell.device()
    dev.set_option("denoise_variance", 1)
    p = cornell.hjr_params(W, H, SPP)
    if a.trace_run:
        dev.set_option("upscale_guided", 1)
        for _ in range(3):
            dev.render_denoised(p, UP, OW, OH)
        dev.close()
        return
    L = hjr.lib()

    # ---- whole frames through the stateful call
    frame_ms = {"option_off": [], "option_on": []}
    for r in range(a.repeats + 1):
        for name, value in (("option_off", 0), ("option_on", 1)):
            dev.set_option("upscale_guided", value)
            t0 = time.perf_counter()
            dev.render_denoised(p, UP, OW, OH)
            if r:
                frame_ms[name].append((time.perf_counter() - t0) * 1e3)
    dev.set_option("upscale_guided", 0)

    # ---- the stages on device buffers, HIP events on a stream of our own (a NULL stream argument would mean the context's stream, which
    # torch's events do not see)
    side = torch.cuda.Stream()
    stream = side.cuda_stream
    assert stream
    col, alb, nrm, filtered = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    var = torch.empty((H, W), dtype=torch.float32, device="cuda")
    out = torch.empty((OH, OW, 4), dtype=torch.float32, device="cuda")
    g_lo = torch.empty((H * W * 48,), dtype=torch.uint8, device="cuda")
    g_hi = torch.empty((OH * OW * 48,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dev.render_device(p, col.data_ptr(), alb.data_ptr(), nrm.data_ptr(), stream=stream, d_variance=var.data_ptr())
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr()  # noqa: E731
    hi_p = hjr.make_params(OW, OH, 1, cornell.camera)
    cam = p.camera

    def ok(rc):
        assert rc == 0, L.hjr_last_error()

    def filt():
        ok(L.hjr_denoise_var_device(dev._h, hjr.MODE_DENOISE, W, H, ptr(col), ptr(alb), ptr(nrm), ptr(var), ptr(filtered), W, H, stream))

    def filt_bilinear():
        ok(L.hjr_denoise_var_device(dev._h, UP, W, H, ptr(col), ptr(alb), ptr(nrm), ptr(var), ptr(out), OW, OH, stream))

    def gbuf_lo():
        ok(L.hjr_render_gbuffer_device(dev._h, ctypes_ref(p), ptr(g_lo), stream))

    def gbuf_hi():
        ok(L.hjr_render_gbuffer_device(dev._h, ctypes_ref(hi_p), ptr(g_hi), stream))

    def kernel():
        ok(L.hjr_upscale_guided_device(dev._h, W, H, ptr(filtered), ptr(g_lo), ctypes_ref(cam), ptr(g_hi), ptr(out), OW, OH, stream))

    cases = {"five_filter_passes": (filt,), "five_passes_and_bilinear_upscale": (filt_bilinear,), "gbuffer_960x540": (gbuf_lo,), "gbuffer_1920x1080": (gbuf_hi,),
             "guided_kernel": (kernel,), "guided_post_stage": (filt, gbuf_lo, gbuf_hi, kernel)}
    ms = {k: [] for k in cases}
    for r in range(a.repeats + 1):
        for name, calls in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            for fn in calls:
                fn()
            e1.record(side)
            torch.cuda.synchronize()
            if r:
                ms[name].append(e0.elapsed_time(e1))
    med = lambda v: {"median": statistics.median(v), "all": v}  # noqa: E731
    stages = {k: med(v) for k, v in ms.items()}
    stages["bilinear_upscale_by_difference"] = stages["five_passes_and_bilinear_upscale"]["median"] - stages["five_filter_passes"]["median"]
    # what the guided kernel has to move at least once: per output pixel its own record's 32 used bytes and a float4 out; per input pixel a float4 and 32 bytes
    min_bytes = OW * OH * (32 + 16) + W * H * (16 + 32)
    stages["guided_kernel"]["min_bytes"] = min_bytes
    stages["guided_kernel"]["min_bytes_over_time_GBps"] = min_bytes / (stages["guided_kernel"]["median"] * 1e-3) / 1e9
    res = {"what": "guided 2x upscale; MI355X; %d x %d output, %d x %d x %d spp NEE, denoise_variance on; medians of %d, alternating in one process" % (OW, OH, W, H, SPP, a.repeats),
           "frame_wall_clock_ms": {k: med(v) for k, v in frame_ms.items()}, "stages_hip_events_ms": stages}

    if not a.no_quality:
        table = gpu_quality_table(cornell, dev)
        print(format_table(table))
        conds = quality_conditions(table)
        for text, holds in conds:
            print("%s: %s" % (text, "holds" if holds else "FAILS"))
        res["quality_96x64_from_48x32x64spp_ref_4096spp"] = {"table": table, "conditions": [{"text": t, "holds": bool(h)} for t, h in conds]}
    dev.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"frame_wall_clock_ms": {k: v["median"] for k, v in res["frame_wall_clock_ms"].items()},
                      "stages_hip_events_ms": {k: (v["median"] if isinstance(v, dict) else v) for k, v in stages.items()}}, indent=1))


def ctypes_ref(s):
    import ctypes
    return ctypes.byref(s)


if __name__ == "__main__":
    main()
