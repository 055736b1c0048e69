"""tools/adaptive_bench.py [--mode quality|machinery] [--out profiles/adaptive.json] [--repeats R] [--label L]
What adaptive sampling (hjr_set_adaptive, DESIGN.md §4 rule 6) buys and costs on C2: the bundled scene at 1920x1080 x 256 spp NEE, colour +
albedo + normal, rendered in 8 sample passes.  Run on the GPU machine from the repository root.

--mode quality (default), one process, the configurations alternating inside every repeat, after one warm-up frame each:
  plain            the 8-pass frame with adaptive sampling off
  adaptive t       noise_threshold t = 0.05 / 0.08 / 0.1 (min_samples default); the frame ends when no tile is active
  uniform t        a plain 8-pass frame of about the samples `adaptive t` rendered (spp = its share x 256 rounded to a multiple of 8)
  per configuration: kernel_ms (sum over the passes of hjr_stats.last_kernel_ms: HIP events around tile order + filter + render +
  accumulate), wall_ms (host wall time of the frame, read-backs and waits included), passes run, share of the 256 spp samples rendered,
  RMSE and relative RMSE |a - ref| / (ref + 0.01) of the colour against a 4096 spp one-shot frame of the exact kernels.
--mode machinery: the cost of the machinery, for alternating runs of this library and of another build (HJR_LIB=...): the plain 8-pass
  frame, and (only when the library has hjr_set_adaptive) the adaptive frame with noise_threshold 1e-30, which stops exactly constant
  tiles only.  Appends one row per run, tagged --label, to the "machinery" list of the output file.
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
import __graft_entry__ as entry  # noqa: E402

hjr = entry.load_package()
W, H, SPP, PASSES = 1920, 1080, 256, 8


class Bench:
    def __init__(self):
        import torch
        self.torch = torch
        cwd = os.getcwd()
        os.chdir(hjr.ASSETS)
        try:
            self.opt = hjr.load_render_option("render_option_c2.json")
            self.scene = hjr.Scene(self.opt.gltf_path.decode(), self.opt.gltf_name.decode(), self.opt)
            lut = self.opt.LUT_path.decode()
            self.lut = hjr.load_png(lut) if lut and os.path.exists(lut) else None
        finally:
            os.chdir(cwd)
        t = 1 / float(self.opt.fps)
        self.cam = self.scene.camera(self.opt, t)
        arrays = self.scene.arrays(t)
        self.dev = hjr.Device(0)
        self.dev.upload_scene(self.scene.view)
        if self.lut is not None:
            self.dev.set_lut(self.lut)
        self.dev.set_transforms(arrays["transforms"], arrays["inv_transforms"])
        self.bufs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
        self.ptrs = [b.data_ptr() for b in self.bufs]
        self.stream = torch.cuda.current_stream().cuda_stream
        self.tiles = ((W + 7) // 8) * ((H + 7) // 8)

    def params(self, spp):
        return hjr.make_params(W, H, spp, self.cam, frame=1, seed=self.opt.seed, integrator=hjr.INTEGRATOR_NEE,
                               sky=tuple(self.opt.scene_sky_default), ibl_intensity=self.opt.IBL_intensity)

    def frame(self, spp, threshold):
        """One frame in 8 passes; threshold None: adaptive sampling off.  Returns kernel ms, wall ms, passes run, samples rendered."""
        if hasattr(self.dev, "set_adaptive"):
            self.dev.set_adaptive(threshold or 0.0)
        p = self.params(spp)
        kernel, n_pass, samples = 0.0, 0, W * H * spp
        t0 = time.perf_counter()
        for b, e in hjr.pass_bounds(spp, PASSES):
            q = hjr.ParamsV2.from_buffer_copy(p)
            q.sample_begin, q.sample_end = b, e
            self.dev.render_device(q, *self.ptrs, stream=self.stream)
            kernel += self.dev.stats()["last_kernel_ms"]
            n_pass += 1
            if threshold:
                st = self.dev.adaptive_state()
                samples = st["samples_rendered"]
                if st["active_tiles"] == 0:
                    break
        self.torch.cuda.synchronize()
        return kernel, 1e3 * (time.perf_counter() - t0), n_pass, samples

    def color(self):
        return self.bufs[0].cpu().numpy()[..., :3].astype(np.float64)


def errors(a, ref):
    d = a - ref
    return float(np.sqrt(np.mean(d * d))), float(np.sqrt(np.mean((d / (ref + 0.01)) ** 2)))


def summarise(rows):
    k = [r[0] for r in rows]
    w = [r[1] for r in rows]
    return {"kernel_ms": statistics.median(k), "kernel_ms_all": [round(v, 3) for v in k], "wall_ms": statistics.median(w),
            "wall_ms_all": [round(v, 3) for v in w], "passes_run": rows[-1][2], "samples_rendered": int(rows[-1][3]),
            "kernel_ms_per_pass": statistics.median(k) / rows[-1][2]}


def quality(b, repeats):
    dev = b.dev
    dev.set_adaptive(0.0)
    ref_p = b.params(4096)
    dev.render_device(ref_p, *b.ptrs, stream=b.stream)
    b.torch.cuda.synchronize()
    ref = b.color()
    full = b.tiles * 64 * SPP  # what the library counts: whole tiles
    configs = [("plain", SPP, None)]
    for t in (0.05, 0.08, 0.1):
        configs.append(("adaptive %g" % t, SPP, t))
    rows = {name: [] for name, _, _ in configs}
    for name, spp, t in list(configs):  # warm-up: buffers, tile lists; and the sample counts that size the uniform frames
        r = b.frame(spp, t)
        if t:
            u = max(8, int(round(r[3] / full * SPP / 8.0)) * 8)
            configs.append(("uniform %g" % t, u, None))
    for name, spp, t in configs[len(rows):]:
        rows[name] = []
        b.frame(spp, t)
    img = {}
    for _ in range(repeats):
        for name, spp, t in configs:
            rows[name].append(b.frame(spp, t))
            if name not in img:
                img[name] = errors(b.color(), ref)
    out = {"width": W, "height": H, "spp": SPP, "passes": PASSES, "integrator": "NEE", "aovs": "color+albedo+normal", "reference_spp": 4096,
           "configs": []}
    for name, spp, t in configs:
        s = summarise(rows[name])
        s.update(name=name, spp=spp, noise_threshold=t, share_of_samples=s["samples_rendered"] / float(W * H * SPP if not t else full),
                 rmse=img[name][0], rel_rmse=img[name][1])
        out["configs"].append(s)
        print("%-14s spp %3d  kernel %7.2f ms  wall %7.2f ms  passes %d  samples %5.1f %%  rmse %.5f  rel rmse %.4f" % (
            name, spp, s["kernel_ms"], s["wall_ms"], s["passes_run"], 100 * s["share_of_samples"], s["rmse"], s["rel_rmse"]), flush=True)
    return out


def machinery(b, repeats, label):
    configs = [("plain", None)] + ([("adaptive 1e-30", 1e-30)] if hasattr(b.dev, "set_adaptive") else [])
    rows = {name: [] for name, _ in configs}
    for name, t in configs:
        b.frame(SPP, t)
    for _ in range(repeats):
        for name, t in configs:
            rows[name].append(b.frame(SPP, t))
    out = {"label": label, "library": hjr.LIB_PATH}
    for name, _ in configs:
        out[name] = summarise(rows[name])
        print("%s %-14s kernel %7.2f ms (%.2f per pass)  wall %7.2f ms  passes %d" % (label, name, out[name]["kernel_ms"], out[name]["kernel_ms_per_pass"],
                                                                                out[name]["wall_ms"], out[name]["passes_run"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("quality", "machinery"), default="quality")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="this")
    a = ap.parse_args()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    b = Bench()
    if a.mode == "quality":
        doc["quality"] = quality(b, a.repeats)
    else:
        doc.setdefault("machinery", []).append(machinery(b, a.repeats, a.label))
    doc["note"] = ("kernel_ms: median over frames of the summed HIP-event time of the passes; wall_ms: median host wall time of a frame, the "
                   "4-byte read-back and the wait for it included; share_of_samples of adaptive rows counts whole 8x8 tiles")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
