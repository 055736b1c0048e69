"""tools/device_bvh_instances_bench.py [--out profiles/device_bvh_instances.json] [--frames 16] -- per-instance trees under a per-commit top
tree (option "device_bvh_instances") against a full device build every frame and against refitting, on the scene and the 16-frame
motion of tools/device_bvh_refit_bench.py (1 M-triangle stress scene, 1920x1080 NEE at 64 and at 8 spp).  Run on the GPU machine from
the repository root.

Configurations, all in this process on the same transforms (device_bvh 1, device_bvh_opt 1):
  rebuild        a full build every frame
  refit_default  device_bvh_refit 1000 with the default growth guard
  instances      device_bvh_instances 1: the topology once (bvh_topology_ms), flatten + boxes + top tree + collapse every frame
Per frame: hjr_stats.frame_build_ms (the commit's kernels, HIP-event time) and the wall time of hjr_set_transforms, bvh_topology_ms,
bvh_instances, bvh_refits, bvh_sah, the render kernel time at 64 and at 8 spp (median of 3 launches), node steps per closest ray.
Derived per configuration: commit + render over the frames at 64 and at 8 spp, bvh_sah at frames 0, 7 and 15, node steps at the last frame.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import device_bvh_refit_bench as rb  # noqa: E402  (the scene's motion and the package)

hjr = rb.hjr
W, H = rb.W, rb.H
CONFIGS = {"rebuild": {}, "refit_default": {"device_bvh_refit": 1000}, "instances": {"device_bvh_instances": 1}}


def run(scene, arrays, cam, opt, options, frames):
    d = hjr.Device(0)
    out = []
    try:
        for k, v in dict({"device_bvh": 1, "device_bvh_opt": 1, "force_rebuild": 1}, **options).items():
            d.set_option(k, v)
        d.upload_scene(scene.view)
        d.set_transforms(*rb.motion(arrays, 0))  # warm-up: allocations, the scene upload
        d.upload_scene(scene.view)               # ... and frame 0 is a full build (and a topology build) in every configuration
        mk = lambda spp, flags=0: hjr.make_params(W, H, spp, cam, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity, flags=flags)  # noqa: E731
        for k in range(frames):
            m, inv = rb.motion(arrays, k)
            t0 = time.perf_counter()
            d.set_transforms(m, inv)
            wall = 1e3 * (time.perf_counter() - t0)
            st = d.stats()
            row = {"frame": k, "build_ms": st["frame_build_ms"], "commit_wall_ms": wall, "bvh_topology_ms": st["bvh_topology_ms"],
                   "bvh_instances": st["bvh_instances"], "bvh_refits": st["bvh_refits"], "bvh_sah": st["bvh_sah"], "bvh_nodes": st["bvh_nodes"]}
            for spp in (64, 8):
                ms = []
                for _ in range(3):
                    d.render(mk(spp), want_aovs=False)
                    ms.append(d.stats()["last_kernel_ms"])
                row["render_ms_%dspp" % spp] = statistics.median(ms)
            d.render(mk(8, hjr.FLAG_STATS), want_aovs=False)
            c = d.stats()
            row["node_steps"] = c["box_tests_closest"] / max(c["closest_rays"], 1)
            out.append(row)
    finally:
        d.close()
    return out


def derive(rows):
    d = {"commit_ms_median": statistics.median(r["build_ms"] for r in rows[1:]), "commit_wall_ms_median": statistics.median(r["commit_wall_ms"] for r in rows[1:]),
         "commit_wall_ms_total": sum(r["commit_wall_ms"] for r in rows), "bvh_topology_ms": rows[-1]["bvh_topology_ms"],
         "bvh_sah": {str(k): rows[k]["bvh_sah"] for k in (0, 7, 15) if k < len(rows)}, "node_steps_last_frame": rows[-1]["node_steps"]}
    for spp in (64, 8):
        key = "render_ms_%dspp" % spp
        d["render_ms_total_%dspp" % spp] = sum(r[key] for r in rows)
        d["commit_plus_render_ms_total_%dspp" % spp] = d["commit_wall_ms_total"] + d["render_ms_total_%dspp" % spp]
        d["render_ms_%dspp" % spp] = {str(k): rows[k][key] for k in (0, 7, 15) if k < len(rows)}
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_bvh_instances.json"))
    ap.add_argument("--frames", type=int, default=16)
    a = ap.parse_args()
    work = tempfile.mkdtemp()
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_stress_scene.py"), work], stdout=subprocess.DEVNULL)
    opt = hjr.load_render_option(os.path.join(work, "render_option_stress.json"))
    scene = hjr.Scene(opt.gltf_path.decode(), opt.gltf_name.decode(), opt)
    t = float(1.0 / opt.fps)
    arrays = scene.arrays(t)
    cam = scene.camera(opt, t)
    res = {"scene": {"triangles": int(scene.view.n_triangles), "instances": int(scene.view.n_instances), "width": W, "height": H, "integrator": "NEE",
                     "frames": a.frames}, "configs": {}, "derived": {}}
    for name, options in CONFIGS.items():
        rows = res["configs"][name] = run(scene, arrays, cam, opt, options, a.frames)
        res["derived"][name] = derive(rows)
        print(name, json.dumps(res["derived"][name]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
