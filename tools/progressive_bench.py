"""tools/progressive_bench.py [--out profiles/progressive.json] [--repeats R] [--variance] -- the cost of rendering a frame in sample passes
(hjr_params.sample_begin / sample_end).  Run on the GPU machine from the repository root.

Two workloads, each rendered in 1, 2, 4, 8 and 32 passes split by hjr.pass_bounds (passes that come out empty are dropped, so the
stress scene's 8 chunks give at most 8 passes):
  c2      the bundled scene at C2 size (render_option_c2.json): 1920x1080 x 256 spp NEE, colour + albedo + normal
  stress  the 1.03 M-triangle scene of tools/make_stress_scene.py (as tools/device_bvh_bench.py): 1920x1080 x 64 spp NEE, colour only
Per pass count, after one warm-up frame, R frames each of:
  kernel_ms        sum over the passes of hjr_stats.last_kernel_ms (HIP events around tile order + render + finalize / accumulate)
  wall_ms          host wall time of the frame: every pass enqueued with hjr_render_device into device tensors, one synchronize at the end
  chunk_bytes      peak chunk-sum bytes (owned tiles x 64 x 16 B x the largest pass's chunks x AOVs) and running-sum bytes (x AOVs when
                   the frame has more than one pass), from the library's allocation rule (csrc/hjr_render.hip::bind_params)
The last pass's colour is checked bit for bit against the one-pass frame.
--variance: every render also writes the variance AOV (a fourth device tensor, one float per pixel; DESIGN.md §4 rule 7).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

hjr = entry.load_package()
PASSES = (1, 2, 4, 8, 32)


def chunk_spp(spp):
    return 8 * (((spp + 7) // 8 + 63) // 64)


def measure(dev, p, n_pass, aovs, repeats, variance):
    import torch
    W, H = p.width, p.height
    bufs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3 if aovs else 1)]
    ptrs = [b.data_ptr() for b in bufs] + [None] * (3 - len(bufs))
    var = torch.empty((H, W), dtype=torch.float32, device="cuda") if variance else None
    stream = torch.cuda.current_stream().cuda_stream
    bounds = hjr.pass_bounds(p.spp, n_pass)

    def frame(with_stats):
        ms = 0.0
        for b, e in bounds:
            q = hjr.ParamsV2.from_buffer_copy(p)
            if len(bounds) > 1:
                q.sample_begin, q.sample_end = b, e
            dev.render_device(q, *ptrs, stream=stream, d_variance=var.data_ptr() if variance else None)
            if with_stats:
                ms += dev.stats()["last_kernel_ms"]
        torch.cuda.synchronize()
        return ms

    frame(False)  # warm-up (buffers, tile lists)
    walls, kernels = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        frame(False)
        walls.append(1e3 * (time.perf_counter() - t0))
        kernels.append(frame(True))
    g = chunk_spp(p.spp)
    owned = ((W + 7) // 8) * ((H + 7) // 8)
    n_aov = len(bufs)
    max_chunks = max((e - b + g - 1) // g for b, e in bounds)
    return {"passes": len(bounds), "bounds": bounds,
            "kernel_ms": statistics.median(kernels), "kernel_ms_all": [round(k, 3) for k in kernels],
            "wall_ms": statistics.median(walls), "wall_ms_all": [round(w, 3) for w in walls],
            "chunk_sum_bytes": owned * 64 * 16 * max_chunks * n_aov,
            "running_sum_bytes": owned * 64 * 16 * n_aov if len(bounds) > 1 else 0,
            "color": bufs[0].cpu().numpy()}


def workload(name, scene, arrays, cam, opt, spp, aovs, repeats, variance):
    dev = hjr.Device(0)
    try:
        dev.upload_scene(scene.view)
        lut = opt.LUT_path.decode()
        if lut and os.path.exists(lut):
            dev.set_lut(hjr.load_png(lut))
        dev.set_transforms(arrays["transforms"], arrays["inv_transforms"])
        p = hjr.make_params(1920, 1080, spp, cam, frame=1, seed=opt.seed, integrator=hjr.INTEGRATOR_NEE,
                            sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)
        rows, ref = [], None
        for n in PASSES:
            r = measure(dev, p, n, aovs, repeats, variance)
            col = r.pop("color")
            if ref is None:
                ref = col
            r["bitexact_vs_one_pass"] = bool((col.view("u4") == ref.view("u4")).all())
            r["requested_passes"] = n
            rows.append(r)
            print("%s: %2d passes  kernel %.2f ms  wall %.2f ms  chunk sums %.1f MB  running sums %.1f MB  bit-exact %s" % (
                name, r["passes"], r["kernel_ms"], r["wall_ms"], r["chunk_sum_bytes"] / 2**20, r["running_sum_bytes"] / 2**20,
                r["bitexact_vs_one_pass"]), flush=True)
        base = rows[0]
        for r in rows:
            extra = r["passes"] - 1
            r["kernel_overhead_ms_per_extra_pass"] = (r["kernel_ms"] - base["kernel_ms"]) / extra if extra else None
            r["wall_overhead_ms_per_extra_pass"] = (r["wall_ms"] - base["wall_ms"]) / extra if extra else None
        return {"width": 1920, "height": 1080, "spp": spp, "integrator": "NEE", "aovs": ("color+albedo+normal" if aovs else "color") + ("+variance" if variance else ""),
                "granule": hjr.sample_granule(spp), "rows": rows}
    finally:
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progressive.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--variance", action="store_true")
    a = ap.parse_args()
    out = {}
    cwd = os.getcwd()
    os.chdir(hjr.ASSETS)
    try:
        opt = hjr.load_render_option("render_option_c2.json")
        scene = hjr.Scene(opt.gltf_path.decode(), opt.gltf_name.decode(), opt)
        t = 1 / float(opt.fps)
        out["c2"] = workload("c2", scene, scene.arrays(t), scene.camera(opt, t), opt, 256, True, a.repeats, a.variance)
    finally:
        os.chdir(cwd)
    work = tempfile.mkdtemp()
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_stress_scene.py"), work], stdout=subprocess.DEVNULL)
    opt = hjr.load_render_option(os.path.join(work, "render_option_stress.json"))
    scene = hjr.Scene(opt.gltf_path.decode(), opt.gltf_name.decode(), opt)
    t = 1 / float(opt.fps)
    out["stress"] = workload("stress", scene, scene.arrays(t), scene.camera(opt, t), opt, 64, False, a.repeats, a.variance)
    out["stress"]["triangles"] = int(scene.view.n_triangles)
    out["note"] = ("kernel_ms: median over frames of the summed HIP-event time of the passes; wall_ms: median host wall time of a frame "
                   "(all passes enqueued, one synchronize); overheads are per extra pass against the one-pass frame")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
