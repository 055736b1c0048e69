#!/usr/bin/env python3
"""tools/denoise_var_bench.py [--out profiles/denoise_var.json] [--repeats 5]
What the variance AOV and the variance-guided filter (hjr_render_var / hjr_denoise_var, DESIGN.md §4 rule 7, §11) cost and buy.  Run on
the GPU machine from the repository root.

  filter   1920 x 1080, the AOVs of one C2 frame on the device: time of hjr_denoise_device and of hjr_denoise_var_device (Denoise mode,
           5 passes each), HIP events around the calls on the stream they run on, median of the repeats after one warm-up call each.
  frame    the C2 frame (bundled scene, 1920 x 1080 x 256 spp NEE, colour + albedo + normal) with and without the variance AOV:
           hjr_stats.last_kernel_ms (HIP events around tile order + render + finalize), alternating, median of the repeats.
  quality  the setup of tests/test_gpu_denoise_var.py::test_quality_error_falls_with_the_sample_count (96 x 64, camera at x = 3.5,
           reference 16384 spp of another seed): e_raw, e_plain, e_var and e_var / e_raw at 16, 64, 256, 1024 spp, and the same from the
           scene's own camera position (where 48 % of the frame is background and the mask keeps about half of the pixels).
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
W, H, SPP = 1920, 1080, 256


def load(config):
    cwd = os.getcwd()
    os.chdir(hjr.ASSETS)
    try:
        opt = hjr.load_render_option(config)
        scene = hjr.Scene(opt.gltf_path.decode(), opt.gltf_name.decode(), opt)
        lut = opt.LUT_path.decode()
        lut = hjr.load_png(lut) if lut and os.path.exists(lut) else None
    finally:
        os.chdir(cwd)
    t = 1 / float(opt.fps)
    arrays = scene.arrays(t)
    dev = hjr.Device(0)
    dev.upload_scene(scene.view)
    if lut is not None:
        dev.set_lut(lut)
    dev.set_transforms(arrays["transforms"], arrays["inv_transforms"])
    return opt, scene, scene.camera(opt, t), dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_var.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    opt, scene, cam, dev = load("render_option_c2.json")
    L = hjr.lib()
    side = torch.cuda.Stream()  # a stream of our own: a NULL stream argument would mean the context's stream, which torch's events do not see
    stream = side.cuda_stream
    assert stream
    kw = dict(frame=1, seed=opt.seed, integrator=hjr.INTEGRATOR_NEE, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)
    p = hjr.make_params(W, H, SPP, cam, **kw)
    col, alb, nrm, out = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    var = torch.empty((H, W), dtype=torch.float32, device="cuda")

    # ---- frame: with / without the variance AOV, alternating
    frame_ms = {"without_variance": [], "with_variance": []}
    for r in range(a.repeats + 1):
        for name, dv in (("without_variance", None), ("with_variance", var.data_ptr())):
            dev.render_device(p, col.data_ptr(), alb.data_ptr(), nrm.data_ptr(), stream=stream, d_variance=dv)
            torch.cuda.synchronize()
            if r:
                frame_ms[name].append(dev.stats()["last_kernel_ms"])

    # ---- filter: plain / variance-guided on that frame's AOVs
    def plain():
        rc = L.hjr_denoise_device(dev._h, hjr.MODE_DENOISE, W, H, col.data_ptr(), alb.data_ptr(), nrm.data_ptr(), out.data_ptr(), W, H, stream)
        assert rc == 0, L.hjr_last_error()

    def guided():
        rc = L.hjr_denoise_var_device(dev._h, hjr.MODE_DENOISE, W, H, col.data_ptr(), alb.data_ptr(), nrm.data_ptr(), var.data_ptr(), out.data_ptr(), W, H, stream)
        assert rc == 0, L.hjr_last_error()
    filter_ms = {"plain": [], "variance_guided": []}
    for r in range(a.repeats + 1):
        for name, fn in (("plain", plain), ("variance_guided", guided)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            fn()
            e1.record(side)
            torch.cuda.synchronize()
            if r:
                filter_ms[name].append(e0.elapsed_time(e1))
    dev.close()

    # ---- quality (the test's setup)
    opt, scene, cam1, dev = load("render_option_c1.json")
    kw = dict(sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)
    quality = {}
    for label, x in (("camera_x_3.5", 3.5), ("camera_of_the_scene", None)):
        cam = hjr.Camera.from_buffer_copy(cam1)
        if x is not None:
            cam.pos[0] = x
        ref = dev.render(hjr.make_params(96, 64, 16384, cam, seed=7, **kw), want_aovs=False)[0]
        mask = (ref[..., :3].max(axis=-1) < 3.0) & (np.abs(ref[..., :3] - 0.8).max(axis=-1) > 1e-3)

        def rmse(img):
            return float(np.sqrt(np.mean((img[..., :3][mask].astype(np.float64) - ref[..., :3][mask]) ** 2)))
        rows = []
        for spp in (16, 64, 256, 1024):
            c, al, n, v = dev.render(hjr.make_params(96, 64, spp, cam, seed=1, **kw), want_variance=True)
            e_raw, e_plain, e_var = rmse(c), rmse(dev.denoise(hjr.MODE_DENOISE, c, al, n)), rmse(dev.denoise(hjr.MODE_DENOISE, c, al, n, variance=v))
            rows.append({"spp": spp, "e_raw": e_raw, "e_plain": e_plain, "e_var": e_var, "e_var_over_e_raw": e_var / e_raw})
        quality[label] = {"mask_share": float(mask.mean()), "rows": rows}
    dev.close()

    res = {
        "what": "variance AOV and variance-guided a-trous filter; MI355X; medians of %d" % a.repeats,
        "filter_1080p_ms": {k: {"median": statistics.median(v), "all": v} for k, v in filter_ms.items()},
        "c2_frame_kernel_ms": {k: {"median": statistics.median(v), "all": v} for k, v in frame_ms.items()},
        "quality_96x64_nee_ref_16384spp": quality,
    }
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
