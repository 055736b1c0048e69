#!/usr/bin/env python3
"""tools/adaptive_temporal_bench.py [--out profiles/adaptive_temporal.json] [--repeats 5] [--trace-only]
What adaptive sampling that counts the temporal history (option "adaptive_temporal", DESIGN.md §4 rule 11 and §11.10) buys and costs.  Run
on the GPU machine from the repository root.

  quality  sequences S (static) and M (every instance moved by frame * (0.05, -0.03, 0.02)) of §11.2: the bundled box from x = 3.5,
           96 x 64, frames 1..8, 256 spp in passes of 32, noise_threshold 0.08, min_samples 32, NEE, Render_mode Denoise; reference 4096 spp
           of seed 7 per frame's geometry and the mask of §11.2.  Per frame the samples rendered and the RMSE of the filtered output of
           three arms: adaptive   hjr_set_adaptive with "denoise_variance" (adaptive sampling as it was: no history)
                       temporal   "denoise_temporal", every frame at full spp  (temporal accumulation as it was)
                       both       "denoise_temporal" + "adaptive_temporal"      (the new option)
           and, per frame with a history, whether every tile's n_tile of `both` is <= rule 6's on the same frame (property (b): the
           `adaptive` arm renders the same frames with the same passes, so its tile_samples are rule 6's).
  prior    1920 x 1080, the C2 scene: hjr_temporal_prior_device against hjr_temporal_accumulate_device (hjr_temporal_kernel<false, false>),
           previous = the current frame's data with a history of 5 everywhere; HIP events around each call on its stream, the two calls
           alternating in one loop, median of the repeats after one warm-up call each.
  passes   1920 x 1080 x 64 spp of the same scene in passes of 16 through hjr_render_denoised, frames 2.. of two contexts in one process
           that render the same frames in turn, one with the option: hjr_stats.last_kernel_ms (HIP events around order + render + finalize
           + decision) summed over the frame's passes, and the samples rendered.
  --trace-only runs the `passes` part alone, for a kernel trace taken around this tool (a run of its own: the decision launch against the
           adaptive finalize dispatch, per kernel; profiles/adaptive_temporal_kernel_stats.csv)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from denoise_var_bench import load  # noqa: E402
from scene_util import Cornell, hjr  # noqa: E402
from temporal_util import camera_at, moved_consistent, ref_mask, rmse  # noqa: E402

QW, QH, QSPP, QSTEP, QTHR, QMS, QFRAMES, QREF = 96, 64, 256, 32, 0.08, 32, 8, 4096
W, H, SPP, STEP = 1920, 1080, 64, 16
MODE = hjr.MODE_DENOISE


def with_range(p, b, e):
    q = hjr.ParamsV2.from_buffer_copy(p)
    q.sample_begin, q.sample_end = b, e
    return q


def adaptive_frame(dev, p, step):
    """The frame in passes of `step` until no tile is active: (filtered image, tile_samples, samples rendered, kernel ms)."""
    ms = 0.0
    for b in range(0, p.spp, step):
        img = dev.render_denoised(with_range(p, b, min(b + step, p.spp)), MODE)
        ms += dev.stats()["last_kernel_ms"]
        st = dev.adaptive_state()
        if st["active_tiles"] == 0:
            break
    return img, dev.tile_samples(), st["samples_rendered"], ms


def quality():
    cornell = Cornell()
    cam = camera_at(cornell, x=3.5)
    kw = dict(sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)
    res = {}
    for name, static in (("S", True), ("M", False)):
        arms = {"adaptive": cornell.device(), "temporal": cornell.device(), "both": cornell.device()}
        arms["adaptive"].set_option("denoise_variance", 1)
        arms["adaptive"].set_adaptive(QTHR, QMS)
        arms["temporal"].set_option("denoise_temporal", 1)
        arms["both"].set_option("denoise_temporal", 1)
        arms["both"].set_option("adaptive_temporal", 1)
        arms["both"].set_adaptive(QTHR, QMS)
        t = {arm: {"samples": [], "rmse": []} for arm in arms}
        t["property_b"] = []
        ref = None
        for f in range(1, QFRAMES + 1):
            xf = moved_consistent(cornell.arrays, 0 if static else f)
            for d in arms.values():
                d.set_transforms(*xf)
            if ref is None or not static:
                ref = arms["temporal"].render(hjr.make_params(QW, QH, QREF, cam, seed=7, **kw), want_aovs=False)[0]
            mask = ref_mask(ref)
            p = hjr.make_params(QW, QH, QSPP, cam, frame=f, seed=1, **kw)
            img6, n6, s6, _ = adaptive_frame(arms["adaptive"], p, QSTEP)
            img11, n11, s11, _ = adaptive_frame(arms["both"], p, QSTEP)
            full = arms["temporal"].render_denoised(p, MODE)
            for arm, img, s in (("adaptive", img6, s6), ("temporal", full, int(n6.size) * 64 * QSPP), ("both", img11, s11)):
                t[arm]["samples"].append(int(s))
                t[arm]["rmse"].append(rmse(img, ref, mask))
            t["property_b"].append(bool((n11 <= n6).all()))
            print("%s frame %d: samples %d / %d / %d, rmse %.5f / %.5f / %.5f, n_tile(both) <= n_tile(rule 6): %s" % (
                name, f, t["adaptive"]["samples"][-1], t["temporal"]["samples"][-1], t["both"]["samples"][-1], t["adaptive"]["rmse"][-1], t["temporal"]["rmse"][-1],
                t["both"]["rmse"][-1], t["property_b"][-1]), flush=True)
        for d in arms.values():
            d.close()
        res[name] = t
    return res


def prior_cost(repeats):
    import torch
    opt, scene, cam, dev = load("render_option_c2.json")
    L = hjr.lib()
    side = torch.cuda.Stream()
    stream = side.cuda_stream
    kw = dict(seed=opt.seed, integrator=hjr.INTEGRATOR_NEE, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)
    p = hjr.make_params(W, H, 16, cam, frame=1, **kw)
    col, alb, nrm, acc, prior = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(5))
    var, acc_var, acc_hist = (torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(3))
    hist = torch.full((H, W), 5.0, dtype=torch.float32, device="cuda")
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

    def accumulate():
        assert L.hjr_temporal_accumulate_device(dev._h, C.byref(fr), C.byref(fr), acc.data_ptr(), acc_var.data_ptr(), acc_hist.data_ptr(), stream) == 0, L.hjr_last_error()

    def prior_call():
        assert L.hjr_temporal_prior_device(dev._h, C.byref(fr), C.byref(fr), prior.data_ptr(), stream) == 0, L.hjr_last_error()
    calls = (("accumulate", accumulate), ("prior", prior_call))
    ms = {name: [] for name, _ in calls}
    for r in range(repeats + 1):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            fn()
            e1.record(side)
            torch.cuda.synchronize()
            if r:
                ms[name].append(e0.elapsed_time(e1))
    carried = float((prior[..., 2] < 1).float().mean().item())
    dev.close()
    return {"kernel_1080p_ms": {k: {"median": statistics.median(v), "all": v} for k, v in ms.items()}, "pixels_with_a_prior": carried}


def pass_cost(repeats):
    opt, scene, cam, off = load("render_option_c2.json")
    _, _, _, on = load("render_option_c2.json")
    kw = dict(seed=opt.seed, integrator=hjr.INTEGRATOR_NEE, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)
    for d, v in ((off, 0), (on, 1)):
        d.set_option("denoise_temporal", 1)
        d.set_option("adaptive_temporal", v)
        d.set_adaptive(QTHR, 16)
    t = {"rule_6": {"kernel_ms": [], "samples": []}, "rule_11": {"kernel_ms": [], "samples": []}}
    for r in range(repeats + 1):
        p = hjr.make_params(W, H, SPP, cam, frame=1 + r, **kw)
        for name, d in (("rule_6", off), ("rule_11", on)):
            if name == "rule_6":
                d.temporal_reset()  # (with the option off an adaptive frame never commits: say so explicitly)
            _, _, s, ms = adaptive_frame(d, p, STEP)
            if r:
                t[name]["kernel_ms"].append(ms)
                t[name]["samples"].append(int(s))
    off.close()
    on.close()
    return {k: {"kernel_ms_median": statistics.median(v["kernel_ms"]), "kernel_ms": v["kernel_ms"], "samples": v["samples"]} for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_temporal.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.trace_only:
        print(json.dumps(pass_cost(a.repeats), indent=1))
        return 0
    res = {
        "what": "adaptive sampling that counts the temporal history; MI355X; medians of %d, the calls alternating in one process" % a.repeats,
        "quality_96x64_256spp_passes_of_32_threshold_0.08": quality(),
        "prior_against_accumulate": prior_cost(a.repeats),
        "frame_1080p_64spp_passes_of_16": pass_cost(a.repeats),
    }
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
