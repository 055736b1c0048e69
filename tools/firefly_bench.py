"""tools/firefly_bench.py [--out profiles/firefly_clamp.json] [--repeats R] [--mode cost|bias|all] -- what the firefly clamp (option
"firefly_clamp", DESIGN.md §4 rule 9) costs and what it does to the picture.  Run on the GPU machine from the repository root.

cost   the bundled scene at C2 size (render_option_c2.json: 1920x1080 x 256 spp NEE, colour + albedo + normal): after a warm-up frame of
       each, frames with the option off and with kappa = 4 ALTERNATE in one process, R of each; kernel_ms is hjr_stats.last_kernel_ms (HIP
       events around tile order + render + hjr_finalize_kernel [+ hjr_firefly_kernel]).  The colour of the option-off frame is checked to
       be the same bits before and after the option was on.  The dispatch times of the two chunk-sum kernels alone come from a kernel trace
       of this mode (a profiler run of its own), not from here.
bias   48 x 32, NEE, seed 1, frame 1, at 64 and 256 spp, kappa = 2 / 4 / 8, from a camera at x = 3.5 and from the scene's own, against an
       8192 spp frame of seed 7; pixels of the reference with a channel >= 3, or within 1e-3 of the sky's 0.8, are out.  Per case: RMSE of
       the plain and the clamped frame, energy kept = sum of the clamped frame over the mask / that of the plain frame of the same samples,
       the share of (pixel, chunk) pairs scaled, and where the rule removes real light: pixels whose own median chunk is black have
       lim = eps x g, so every lit chunk of theirs is cut to next to nothing (caustics on dark surfaces).  They are found from the frames
       (the chunk sums stay on the device): pixels that lost energy and whose clamped r + g + b is below 4 x eps; reported are their number
       and their share of the removed energy.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

hjr = entry.load_package()
EPS = 1e-3  # HJR_FIREFLY_EPS


def load(config):
    cwd = os.getcwd()
    os.chdir(hjr.ASSETS)
    try:
        opt = hjr.load_render_option(config)
        scene = hjr.Scene(opt.gltf_path.decode(), opt.gltf_name.decode(), opt)
        t = float(np.float32(1) / np.float32(opt.fps))
        lut = hjr.load_png(opt.LUT_path.decode()) if opt.LUT_path and os.path.exists(opt.LUT_path.decode()) else None
        return opt, scene, scene.arrays(t), scene.camera(opt, t), lut
    finally:
        os.chdir(cwd)


def device(scene, arrays, lut):
    dev = hjr.Device(0)
    dev.upload_scene(scene.view)
    if lut is not None:
        dev.set_lut(lut)
    dev.set_transforms(arrays["transforms"], arrays["inv_transforms"])
    return dev


def cost(repeats):
    import torch
    opt, scene, arrays, cam, lut = load("render_option_c2.json")
    dev = device(scene, arrays, lut)
    try:
        W, H, spp = 1920, 1080, 256
        p = hjr.make_params(W, H, spp, cam, frame=1, seed=opt.seed, integrator=hjr.INTEGRATOR_NEE, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)
        bufs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
        stream = torch.cuda.current_stream().cuda_stream

        def frame(kappa):
            dev.set_option("firefly_clamp", kappa)
            dev.render_device(p, *[b.data_ptr() for b in bufs], stream=stream)
            torch.cuda.synchronize()
            return dev.stats()

        frame(0)
        off0 = bufs[0].cpu().numpy().copy()
        frame(4)
        ms = {0: [], 4: []}
        count = 0
        for _ in range(repeats):
            for kappa in (0, 4):
                st = frame(kappa)
                ms[kappa].append(st["last_kernel_ms"])
                if kappa:
                    count = st["firefly_clamped"]
                else:
                    assert st["firefly_clamped"] == 0
        frame(0)
        same = bool((bufs[0].cpu().numpy().view("u4") == off0.view("u4")).all())
        g = hjr.sample_granule(spp)
        res = {"width": W, "height": H, "spp": spp, "integrator": "NEE", "aovs": "color+albedo+normal", "repeats": repeats,
               "kernel_ms_off": statistics.median(ms[0]), "kernel_ms_off_all": [round(v, 3) for v in ms[0]],
               "kernel_ms_kappa4": statistics.median(ms[4]), "kernel_ms_kappa4_all": [round(v, 3) for v in ms[4]],
               "pairs_scaled": count, "pairs": W * H * (spp // g), "option_off_frame_same_bits_after": same,
               "colour_chunk_sum_bytes": W * H * 16 * (spp // g)}
        res["delta_ms"] = res["kernel_ms_kappa4"] - res["kernel_ms_off"]
        print("cost: off %.3f ms, kappa 4 %.3f ms (delta %+.3f ms), %d of %d pairs scaled, option-off bits unchanged: %s"
              % (res["kernel_ms_off"], res["kernel_ms_kappa4"], res["delta_ms"], count, res["pairs"], same), flush=True)
        return res
    finally:
        dev.close()


def bias():
    opt, scene, arrays, cam, lut = load("render_option_c1.json")
    dev = device(scene, arrays, lut)
    try:
        moved = type(cam).from_buffer_copy(cam)
        moved.pos[0] = 3.5
        rows = []
        for name, c in (("x = 3.5", moved), ("the scene's own", cam)):
            mk = lambda spp, seed: hjr.make_params(48, 32, spp, c, frame=1, seed=seed, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)
            dev.set_option("firefly_clamp", 0)
            ref = dev.render(mk(8192, 7), want_aovs=False)[0][..., :3].astype(np.float64)
            mask = ~((ref >= 3.0).any(-1) | (np.abs(ref - 0.8) < 1e-3).all(-1))
            rmse = lambda img: float(np.sqrt(np.mean(((img - ref)[mask]) ** 2)))
            for spp in (64, 256):
                dev.set_option("firefly_clamp", 0)
                plain = dev.render(mk(spp, 1), want_aovs=False)[0][..., :3].astype(np.float64)
                row = {"camera": name, "spp": spp, "mask_share": float(mask.mean()), "rmse_plain": rmse(plain),
                       "reference_over_plain_sum": float(ref[mask].sum() / plain[mask].sum())}
                for kappa in (2, 4, 8):
                    dev.set_option("firefly_clamp", kappa)
                    img = dev.render(mk(spp, 1), want_aovs=False)[0][..., :3].astype(np.float64)
                    n = dev.stats()["firefly_clamped"]
                    removed = (plain - img).sum(-1)
                    dark = mask & (img.sum(-1) < 4 * EPS) & (removed > 0)
                    row["kappa_%d" % kappa] = {"rmse": rmse(img), "energy_kept": float(img[mask].sum() / plain[mask].sum()),
                                               "pairs_scaled_share": n / (48 * 32 * (spp // 8)),
                                               "removed_in_pixels_left_black_share": float(removed[dark].sum() / removed[mask].sum()) if removed[mask].sum() > 0 else 0.0,
                                               "pixels_left_black": int(dark.sum())}
                rows.append(row)
                print("bias: camera %s, %d spp, mask %.0f %%: RMSE plain %.5f, kappa 2 / 4 / 8 %s, energy kept %s" % (
                    name, spp, 100 * row["mask_share"], row["rmse_plain"], " / ".join("%.5f" % row["kappa_%d" % k]["rmse"] for k in (2, 4, 8)),
                    " / ".join("%.3f" % row["kappa_%d" % k]["energy_kept"] for k in (2, 4, 8))), flush=True)
        return rows
    finally:
        dev.set_option("firefly_clamp", 0)
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "firefly_clamp.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mode", choices=("cost", "bias", "all"), default="all")
    a = ap.parse_args()
    out = {}
    if a.mode in ("bias", "all"):
        out["bias"] = bias()
    if a.mode in ("cost", "all"):
        out["cost"] = cost(a.repeats)
    out["note"] = ("cost: HIP-event kernel time of whole frames, option off and kappa 4 alternating in one process, medians; bias: 48 x 32 NEE frames of "
                   "seed 1 against 8192 spp of seed 7, mask = reference pixels with no channel >= 3 and not within 1e-3 of the sky")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
