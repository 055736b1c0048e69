#!/usr/bin/env python3
"""tools/spatial_var_bench.py [--out profiles/spatial_var.json] [--repeats 5] [--no-quality]
What the spatial variance estimate (hjr_estimate_variance, option "denoise_variance_spatial") costs and buys.  Run on the
GPU machine from the repository root.

  cost     1920 x 1080, the AOVs of one 4 spp frame of the bundled scene on the device (its variance AOV is HJR_VARIANCE_UNKNOWN everywhere).
           What hjr_render_denoised runs behind its render, option off against on, alternating in this process: off = the five passes of
           hjr_denoise_var_device; on = hjr_estimate_variance_device in place, then the same five passes.  HIP events around the calls on
           the stream they run on, median of the repeats after one warm-up round.  The variance buffer is set back to unknown before
           every timed window, outside it.  Also the estimate on its own: every pixel unknown (nine taps each) and every pixel known (one
           read, one write).
  quality  the tables of tests/test_gpu_spatial_var.py from GPU frames (96 x 64, camera at x = 3.5, references of 4096 spp): single frames
           at 1, 2, 4, 8 spp, and the 8-frame temporal chains at 4 spp, static and moving; every filter stage is a CPU checker.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from scene_util import Cornell, hjr  # noqa: E402
from spatial_var_util import (CHAIN_FRAMES, beats_plain_share, format_tables, gpu_single_frame_table, gpu_temporal_chain, lower_median,  # noqa: E402
                              quality_conditions)

W, H, SPP = 1920, 1080, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_var.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-quality", action="store_true")
    a = ap.parse_args()
    import torch
    cornell = Cornell()
    dev = cornell.device()
    L = hjr.lib()
    side = torch.cuda.Stream()  # a stream of our own: a NULL stream argument would mean the context's stream, which torch's events do not see
    stream = side.cuda_stream
    assert stream
    col, alb, nrm, out = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    var, work = (torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    dev.render_device(cornell.hjr_params(W, H, SPP), col.data_ptr(), alb.data_ptr(), nrm.data_ptr(), stream=stream, d_variance=var.data_ptr())
    torch.cuda.synchronize()
    assert bool((var == 1e30).all()), "a 4 spp frame has no variance"
    known = torch.full((H, W), 0.01, dtype=torch.float32, device="cuda")
    ptr = lambda t: t.data_ptr()  # noqa: E731

    def estimate():
        rc = L.hjr_estimate_variance_device(dev._h, W, H, ptr(col), ptr(alb), ptr(nrm), ptr(work), ptr(work), stream)
        assert rc == 0, L.hjr_last_error()

    def guided():
        rc = L.hjr_denoise_var_device(dev._h, hjr.MODE_DENOISE, W, H, ptr(col), ptr(alb), ptr(nrm), ptr(work), ptr(out), W, H, stream)
        assert rc == 0, L.hjr_last_error()

    cases = {"post_stage_option_off": (var, (guided,)), "post_stage_option_on": (var, (estimate, guided)),
             "estimate_all_unknown": (var, (estimate,)), "estimate_all_known": (known, (estimate,))}
    ms = {k: [] for k in cases}
    for r in range(a.repeats + 1):
        for name, (src, calls) in cases.items():
            with torch.cuda.stream(side):
                work.copy_(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            for fn in calls:
                fn()
            e1.record(side)
            torch.cuda.synchronize()
            if r:
                ms[name].append(e0.elapsed_time(e1))
    cost = {k: {"median": statistics.median(v), "all": v} for k, v in ms.items()}
    # the bytes the estimate has to move at least once when every pixel is unknown: three float4 AOVs and a float in, a float out
    cost["estimate_all_unknown"]["min_bytes"] = W * H * (3 * 16 + 4 + 4)
    cost["estimate_all_unknown"]["min_bytes_over_time_GBps"] = W * H * (3 * 16 + 4 + 4) / (cost["estimate_all_unknown"]["median"] * 1e-3) / 1e9
    res = {"what": "spatial variance estimate; MI355X; %d x %d; medians of %d, option off and on alternating in one process" % (W, H, a.repeats),
           "cost_1080p_ms": cost}

    if not a.no_quality:
        table = gpu_single_frame_table(cornell, dev)
        chains = {"static": gpu_temporal_chain(cornell, dev, False), "moving": gpu_temporal_chain(cornell, dev, True)}
        print(format_tables(table, chains))
        conds = quality_conditions(table, chains)
        for text, holds in conds:
            print("%s: %s" % (text, "holds" if holds else "FAILS"))
        res["quality_96x64_nee_ref_4096spp"] = {
            "single_frames": {str(spp): dict(row, lower_median={k: lower_median(v) for k, v in row.items()}) for spp, row in table.items()},
            "temporal_chains_4spp": chains,
            "chain_frames_2_to_%d_below_the_plain_filter" % CHAIN_FRAMES: beats_plain_share(chains),
            "conditions": [{"text": t, "holds": bool(h)} for t, h in conds]}
    dev.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["cost_1080p_ms"], indent=1))


if __name__ == "__main__":
    main()
