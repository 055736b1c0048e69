"""tools/firefly_passes_bench.py [--out profiles/firefly_passes.json] [--repeats R] -- what the firefly clamp on sample passes (option
"firefly_clamp_passes", DESIGN.md §4 rule 10) costs on C2: the bundled scene at 1920x1080 x 256 spp NEE, colour + albedo + normal, rendered
in 8 sample passes.  Run on the GPU machine from the repository root.

One process, the configurations alternating inside every repeat, after one warm-up frame each:
  off            "firefly_clamp" 0: the plain 8-pass frame
  clamp          "firefly_clamp" 4, "firefly_clamp_passes" 1: every pass from the fourth chunk on runs hjr_firefly_kernel<128, true, false>
  adaptive off   hjr_set_adaptive(0.08) with "firefly_clamp" 0: today's adaptive frame
  adaptive clamp ... with both options on: the clamped statistic decides (hjr_firefly_kernel<128, true, true>)
Per configuration: kernel_ms (sum over the passes of hjr_stats.last_kernel_ms: HIP events around tile order + filter + render + finalize
[+ firefly kernel]), the per-pass values of the last repeat, wall_ms, passes run, share of the frame's samples rendered, (pixel, chunk) pairs
scaled in the last pass written, and the RMSE of the colour against a 4096 spp one-shot frame.  The colour of the last `clamp` pass is
checked to be the one-shot clamped frame's bits, and the `off` frame's to be the same bits before and after the options were on.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from adaptive_bench import PASSES, SPP, Bench, H, W, errors, hjr  # noqa: E402

KAPPA, THRESHOLD = 4, 0.08
CONFIGS = [("off", 0, None), ("clamp", KAPPA, None), ("adaptive off", 0, THRESHOLD), ("adaptive clamp", KAPPA, THRESHOLD)]


def frame(b, kappa, threshold):
    """One frame in 8 passes.  Returns (kernel ms, wall ms, passes run, samples rendered, pairs scaled in the last pass, per-pass kernel ms)."""
    dev = b.dev
    dev.set_option("firefly_clamp", kappa)
    dev.set_option("firefly_clamp_passes", 1 if kappa else 0)
    dev.set_adaptive(threshold or 0.0)
    p = b.params(SPP)
    per_pass, samples, pairs = [], W * H * SPP, 0
    t0 = time.perf_counter()
    for begin, end in hjr.pass_bounds(SPP, PASSES):
        q = hjr.ParamsV2.from_buffer_copy(p)
        q.sample_begin, q.sample_end = begin, end
        dev.render_device(q, *b.ptrs, stream=b.stream)
        st = dev.stats()
        per_pass.append(st["last_kernel_ms"])
        pairs = st["firefly_clamped"]
        if threshold:
            a = dev.adaptive_state()
            samples = a["samples_rendered"]
            if a["active_tiles"] == 0:
                break
    b.torch.cuda.synchronize()
    return sum(per_pass), 1e3 * (time.perf_counter() - t0), len(per_pass), samples, pairs, per_pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "firefly_passes.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    b = Bench()
    dev = b.dev
    ref_p = b.params(4096)
    dev.render_device(ref_p, *b.ptrs, stream=b.stream)
    b.torch.cuda.synchronize()
    ref = b.color()
    dev.set_option("firefly_clamp", KAPPA)
    dev.render_device(b.params(SPP), *b.ptrs, stream=b.stream)
    b.torch.cuda.synchronize()
    one_shot = b.bufs[0].cpu().numpy().copy()
    one_shot_pairs = dev.stats()["firefly_clamped"]
    rows = {name: [] for name, _, _ in CONFIGS}
    img, bits_ok = {}, {}
    for name, kappa, t in CONFIGS:  # warm-up: buffers (the kept chunk sums among them), tile lists
        frame(b, kappa, t)
        if name == "off":
            off0 = b.bufs[0].cpu().numpy().copy()
    for _ in range(a.repeats):
        for name, kappa, t in CONFIGS:
            rows[name].append(frame(b, kappa, t))
            if name not in img:
                img[name] = errors(b.color(), ref)
                if name == "clamp":
                    bits_ok["clamp_last_pass_is_one_shot_clamped"] = bool((b.bufs[0].cpu().numpy().view("u4") == one_shot.view("u4")).all())
    frame(b, 0, None)
    bits_ok["off_frame_same_bits_after"] = bool((b.bufs[0].cpu().numpy().view("u4") == off0.view("u4")).all())
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    out = {"width": W, "height": H, "spp": SPP, "passes": PASSES, "integrator": "NEE", "aovs": "color+albedo+normal", "kappa": KAPPA,
           "noise_threshold": THRESHOLD, "reference_spp": 4096, "repeats": a.repeats, "one_shot_pairs_scaled": one_shot_pairs,
           "colour_chunk_sum_bytes_kept": W * H * 16 * (SPP // hjr.sample_granule(SPP)), "configs": []}
    out.update(bits_ok)
    for name, kappa, t in CONFIGS:
        r = rows[name]
        k = [v[0] for v in r]
        s = {"name": name, "kernel_ms": statistics.median(k), "kernel_ms_all": [round(v, 3) for v in k], "wall_ms": statistics.median(v[1] for v in r),
             "passes_run": r[-1][2], "share_of_samples": r[-1][3] / float(W * H * SPP if not t else tiles * 64 * SPP), "pairs_scaled_last_pass": r[-1][4],
             "kernel_ms_per_pass_last_repeat": [round(v, 3) for v in r[-1][5]], "rmse": img[name][0], "rel_rmse": img[name][1]}
        out["configs"].append(s)
        print("%-15s kernel %7.2f ms (%s)  wall %7.2f ms  passes %d  samples %5.1f %%  pairs %d  rmse %.5f" % (
            name, s["kernel_ms"], " ".join("%.2f" % v for v in k), s["wall_ms"], s["passes_run"], 100 * s["share_of_samples"], s["pairs_scaled_last_pass"], s["rmse"]), flush=True)
    print(bits_ok, flush=True)
    out["note"] = ("kernel_ms: median over frames of the summed HIP-event time of the passes, the four configurations alternating in one process; "
                   "share_of_samples of adaptive rows counts whole 8x8 tiles; rmse against a 4096 spp plain frame (the clamp's bias included)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
