#!/usr/bin/env python3
"""tools/denoise_shards_bench.py [--out profiles/denoise_shards.json] [--repeats 5] [--sizes 1920x1080,3840x2160]
What rank 0 pays for a Denoise-mode frame on the multi-GPU path (hjr_assemble_shards_device / hjr_denoise_shards_device, DESIGN.md §7
"Denoise modes").  One GPU, emulated shards: the context renders every rank's packed AOVs of the C2 frame (bundled scene, 256 spp NEE) into
one buffer laid out as the frame's gather leaves it (8 ranks, colour | albedo | normal | variance).  Run on the GPU machine from the
repository root.  Every time is HIP events around the calls on the stream they run on, the median of the repeats after one warm-up.

  assemble   hjr_assemble_shards_kernel (one launch) against what the parent commit does, 8 x 3 hjr_unpack_tiles_device launches, on the
             three float4 AOVs (the variance has no per-rank form); the four-AOV time of the one launch beside it.  The two alternate and
             both runs of each are recorded.
  serial     rank 0's serial share per filter variant (plain, "denoise_variance", "denoise_temporal") in Denoise and DenoiseUpScale2X:
             assemble + (G-buffer + accumulation) + filter + upscale = one hjr_denoise_shards_device call; beside it the C2 render of the
             whole frame measured in the same run (hjr_stats.last_kernel_ms: HIP events around the launch; same median) divided by 8, and the ratio of the two: the bound on 8-GPU
             scaling of a Denoise frame.  Emulated shards on one GPU: not an RCCL measurement.
  gather     bytes per frame, computed: 16 + 16 + 16 + 4 per pixel with the variance, 48 without.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

hjr = entry.load_package()
N, SPP = 8, 256
FILTERS = {"plain": (0, 0), "denoise_variance": (1, 0), "denoise_temporal": (0, 1)}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_shards.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    a = ap.parse_args()
    import torch
    opt, scene, cam, dev = load("render_option_c2.json")
    L = hjr.lib()
    side = torch.cuda.Stream()  # a stream of our own: torch's events do not see the context's stream
    stream = side.cuda_stream
    assert stream
    kw = dict(frame=1, seed=opt.seed, integrator=hjr.INTEGRATOR_NEE, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)

    def timed(fn):
        fn()  # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": statistics.median(ms), "runs_ms": ms}

    def shards(w, h):
        """Every rank's packed AOVs of the w x h C2 frame, rendered in turn into one gathered buffer."""
        off, stride = hjr.shards_layout(w, h, N)
        buf = torch.zeros((stride * N // 4,), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for r in range(N):
            base = buf.data_ptr() + r * stride
            p = hjr.make_params(w, h, SPP, cam, rank=r, world_size=N, flags=hjr.FLAG_PACKED, **kw)
            dev.render_device(p, base + off["color"], base + off["albedo"], base + off["normal"], stream=stream, d_variance=base + off["variance"])
        torch.cuda.synchronize()
        return buf, off, stride

    result = {"gpu": torch.cuda.get_device_name(0), "world_size": N, "spp": SPP, "repeats": a.repeats, "sizes": {}}
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        entry_ = {}
        # ---- the C2 render of the whole frame on this GPU (what one of 8 GPUs renders an eighth of)
        col, alb, nrm = (torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(3))
        var = torch.empty((h, w), dtype=torch.float32, device="cuda")
        render_ms = []
        p_full = hjr.make_params(w, h, SPP, cam, **kw)
        for r in range(a.repeats + 1):  # one warm-up, then the repeats
            dev.render_device(p_full, col.data_ptr(), alb.data_ptr(), nrm.data_ptr(), stream=stream, d_variance=var.data_ptr())
            torch.cuda.synchronize()
            if r:
                render_ms.append(dev.stats()["last_kernel_ms"])
        entry_["render_c2_ms"] = {"median_ms": statistics.median(render_ms), "runs_ms": render_ms}
        share = statistics.median(render_ms) / N

        buf, off, stride = shards(w, h)
        s4 = hjr.make_shards(buf.data_ptr(), N, stride, off)
        s3 = hjr.make_shards(buf.data_ptr(), N, stride, {k: off[k] for k in ("color", "albedo", "normal")})
        block = hjr.owned_tiles(w, h, 0, N) * 64 * 16

        def one_launch(s, with_var):
            def fn():
                rc = L.hjr_assemble_shards_device(dev._h, C.byref(s), w, h, col.data_ptr(), alb.data_ptr(), nrm.data_ptr(), var.data_ptr() if with_var else None, stream)
                assert rc == 0, L.hjr_last_error()
            return fn

        def per_rank_loop():
            for r in range(N):
                for k, dst in (("color", col), ("albedo", alb), ("normal", nrm)):
                    rc = L.hjr_unpack_tiles_device(dev._h, buf.data_ptr() + r * stride + off[k], w, h, r, N, dst.data_ptr(), stream)
                    assert rc == 0, L.hjr_last_error()
        asm = {"one_launch_3_aovs": [], "loop_24_launches_3_aovs": [], "one_launch_4_aovs": []}
        for _ in range(2):  # alternate; both runs of each are kept
            asm["one_launch_3_aovs"].append(timed(one_launch(s3, False)))
            asm["loop_24_launches_3_aovs"].append(timed(per_rank_loop))
            asm["one_launch_4_aovs"].append(timed(one_launch(s4, True)))
        # (the two forms must agree before their times mean anything)
        per_rank_loop()
        torch.cuda.synchronize()
        loop_frames = [t.clone() for t in (col, alb, nrm)]
        one_launch(s4, True)()
        torch.cuda.synchronize()
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(loop_frames, (col, alb, nrm)))
        asm["bytes_moved_3_aovs"] = 2 * 3 * w * h * 16  # read + write
        asm["bytes_moved_4_aovs"] = 2 * (3 * w * h * 16 + w * h * 4)
        entry_["assemble"] = asm

        # ---- rank 0's serial share: one hjr_denoise_shards_device call per filter variant and mode
        serial = {}
        out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        for mode_name, mode in (("Denoise", hjr.MODE_DENOISE), ("DenoiseUpScale2X", hjr.MODE_DENOISE_UPSCALE2X)):
            rw, rh = (w // 2, h // 2) if mode == hjr.MODE_DENOISE_UPSCALE2X else (w, h)
            if (rw, rh) != (w, h):
                mbuf, moff, mstride = shards(rw, rh)
            else:
                mbuf, moff, mstride = buf, off, stride
            ms_ = hjr.make_shards(mbuf.data_ptr(), N, mstride, moff)
            p = hjr.make_params(rw, rh, SPP, cam, **kw)
            for name, (v, t) in FILTERS.items():
                dev.set_option("denoise_variance", v)
                dev.set_option("denoise_temporal", t)

                def fn():
                    rc = L.hjr_denoise_shards_device(dev._h, C.byref(p), mode, C.byref(ms_), out.data_ptr(), w, h, stream)
                    assert rc == 0, L.hjr_last_error()
                r = timed(fn)  # ("denoise_temporal": the warm-up call is the first frame; the timed ones reproject against a history)
                r["render_c2_over_8_ms"] = share
                r["serial_over_parallel"] = r["median_ms"] / share
                serial["%s/%s" % (mode_name, name)] = r
            dev.set_option("denoise_variance", 0)
            dev.set_option("denoise_temporal", 0)
        entry_["serial_share"] = serial
        entry_["gather_bytes_per_frame"] = {"with_variance": w * h * 52, "without_variance": w * h * 48,
                                            "padded_per_rank_with_variance": block // 16 * 52, "note": "computed, not measured"}
        result["sizes"][size] = entry_
        del buf, col, alb, nrm, var, out
        torch.cuda.empty_cache()
    result["note"] = ("one GPU, emulated shards: the ncclGather of the larger payload on N > 1 GPUs is not measured (two ranks need two GPUs); "
                      "serial_over_parallel = rank 0's serial share over one GPU's eighth of the C2 render")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
