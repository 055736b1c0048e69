"""tools/device_bvh_bench.py [--out profiles/device_bvh.json] [--builders a,b,...] -- host vs device per-frame BVH build on the 1 M-triangle
stress scene (tools/make_stress_scene.py defaults), 1920x1080 x 64 spp NEE.  Run on the GPU machine from the repository root.

For each builder (host with bvh_refine 0, host with bvh_refine 1, device_bvh 1, device_bvh 1 with device_bvh_opt 1..3 as device_opt1..3):
  build_ms       median of 5 forced rebuilds after one warm-up: hjr_stats.frame_build_ms (host wall time on 16 threads, device event time)
  render_ms      median kernel time of 3 renders after one warm-up
  node_steps     box_tests_closest / closest_rays of one HJR_FLAG_STATS launch
  loop_ms        per-frame wall time of a serial in-process loop: forced rebuild + render, 4 frames after a warm-up
  sah            BVH4 SAH of the tree (hjr_copy_frame_data: Ci 1.2 per inner slot, Ct 1 per triangle of a leaf slot, by slot area over
                 root area); only for the BVH4 memory layout (lds_mode 0), null otherwise
and for host (default refine) and device: henjou_cli's per-frame wall time of the forced-rebuild animation (serial_io 0, 5 frames).
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

hjr = entry.load_package()
W, H, SPP = 1920, 1080, 64
BUILDERS = {"host_refine0": {"bvh_refine": 0}, "host_refine1": {"bvh_refine": 1}, "device": {"device_bvh": 1},
            "device_opt1": {"device_bvh": 1, "device_bvh_opt": 1}, "device_opt2": {"device_bvh": 1, "device_bvh_opt": 2},
            "device_opt3": {"device_bvh": 1, "device_bvh_opt": 3}}


def bvh4_sah(d):
    import numpy as np
    raw = d.copy_frame_data(hjr.FRAME_NODES).reshape(-1, 7, 4)
    nodes, refs = raw.astype(np.float64), raw[:, 6, :].view(np.uint32)
    lo = np.stack([nodes[:, 0], nodes[:, 2], nodes[:, 4]], -1)
    hi = np.stack([nodes[:, 1], nodes[:, 3], nodes[:, 5]], -1)
    used = refs != 0x80000000
    e = np.maximum(hi - lo, 0.0)
    area = 2.0 * (e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0])
    w = np.where((refs & 0x80000000) != 0, 1.0 * ((refs >> 27) & 15), 1.2)
    r = np.maximum(hi[0][used[0]].max(0) - lo[0][used[0]].min(0), 0.0)
    return float((w * area)[used].sum() / (2.0 * (r[0] * r[1] + r[1] * r[2] + r[2] * r[0])))


def measure(scene, arrays, cam, opt, options):
    d = hjr.Device(0)
    try:
        d.set_option("host_threads", 16)
        for k, v in options.items():
            d.set_option(k, v)
        d.upload_scene(scene.view)
        m, inv = arrays["transforms"], arrays["inv_transforms"]
        d.set_transforms(m, inv)
        d.set_option("force_rebuild", 1)
        builds = []
        for _ in range(5):
            d.set_transforms(m, inv)
            builds.append(d.stats()["frame_build_ms"])
        p = hjr.make_params(W, H, SPP, cam, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)
        d.render(p, want_aovs=False)
        renders = []
        for _ in range(3):
            d.render(p, want_aovs=False)
            renders.append(d.stats()["last_kernel_ms"])
        st = d.stats()
        sah = bvh4_sah(d) if st["lds_mode"] == 0 else None
        ps = hjr.make_params(W, H, SPP, cam, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity, flags=hjr.FLAG_STATS)
        d.render(ps, want_aovs=False)
        cnt = d.stats()
        loop = []
        for _ in range(4):
            t0 = time.perf_counter()
            d.set_transforms(m, inv)
            d.render(p, want_aovs=False)
            loop.append(1e3 * (time.perf_counter() - t0))
        return {"build_ms": statistics.median(builds), "builds_ms": builds, "render_ms": statistics.median(renders),
                "node_steps": cnt["box_tests_closest"] / max(cnt["closest_rays"], 1), "loop_ms": statistics.median(loop),
                "bvh_nodes": st["bvh_nodes"], "bvh_depth": st["bvh_depth"], "stack_need": st["stack_need"], "lds_mode": st["lds_mode"], "sah": sah}
    finally:
        d.close()


def cli_loop(work, device_bvh, frames=5):
    ro = json.load(open(os.path.join(work, "render_option_stress.json")))
    ro["Animation"].update(start_frame=1, end_frame=1 + frames)
    ro["Image"].update(image_width=W, image_height=H, max_spp=SPP)
    ro["Henjou_HIP"] = {"serial_io": False, "force_rebuild": True, "device_bvh": bool(device_bvh)}
    path = os.path.join(work, "ro_cli_%d.json" % device_bvh)
    json.dump(ro, open(path, "w"))
    cli = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
    p = subprocess.run([cli, path], cwd=work, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("henjou_cli failed: " + p.stderr[-2000:])
    m = re.search(r"\(([0-9.]+) ms per frame", p.stderr)
    return float(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_bvh.json"))
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--builders", default=",".join(BUILDERS), help="comma-separated subset of " + ", ".join(BUILDERS))
    a = ap.parse_args()
    work = tempfile.mkdtemp()
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_stress_scene.py"), work], stdout=subprocess.DEVNULL)
    opt = hjr.load_render_option(os.path.join(work, "render_option_stress.json"))
    scene = hjr.Scene(opt.gltf_path.decode(), opt.gltf_name.decode(), opt)
    t = float(1.0 / opt.fps)
    arrays = scene.arrays(t)
    cam = scene.camera(opt, t)
    res = {"scene": {"triangles": int(scene.view.n_triangles), "width": W, "height": H, "spp": SPP, "integrator": "NEE"}, "builders": {}}
    for name in a.builders.split(","):
        res["builders"][name] = measure(scene, arrays, cam, opt, BUILDERS[name])
        print(name, json.dumps(res["builders"][name]), flush=True)
    if not a.skip_cli:
        res["cli_forced_rebuild_ms_per_frame"] = {"host_default": cli_loop(work, 0), "device": cli_loop(work, 1)}
        print("cli", json.dumps(res["cli_forced_rebuild_ms_per_frame"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
