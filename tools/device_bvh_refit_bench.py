"""tools/device_bvh_refit_bench.py [--out profiles/device_bvh_refit.json] [--frames 16] -- refit against rebuild of the device-built BVH on
the 1 M-triangle stress scene (tools/make_stress_scene.py defaults), 1920x1080 NEE at 64 and at 8 spp.  Run on the GPU machine from the
repository root.

The animation: 16 frames in which every instance moves differently (rotation about y by k * (0.01 + 0.003 (i % 7)), translation
k * 0.02 * a per-instance direction).  Configurations, all in this process on the same transforms:
  rebuild_opt1   device_bvh 1, device_bvh_opt 1, a full build every frame
  rebuild_opt0   device_bvh 1, device_bvh_opt 0, a full build every frame (the plain Morton tree)
  refit_always   device_bvh_opt 1 with device_bvh_refit 1000 and device_bvh_refit_growth 10000: frame 0 builds, every other frame refits
  refit_default  device_bvh_opt 1 with device_bvh_refit 1000 and the default growth guard
Per frame: hjr_stats.frame_build_ms (build or refit, HIP-event time) and the wall time of hjr_set_transforms, bvh_refits, bvh_sah, the
render kernel time at 64 and at 8 spp (median of 3 launches), node steps per closest ray (box_tests_closest / closest_rays of one
HJR_FLAG_STATS launch at 8 spp).
Derived (refit_always against rebuild_opt1, frames 1..): the refit time against the build time, render ms per percent of SAH growth
(least squares through the origin), and the growth at which a rebuild pays: (build ms - refit ms) / (render ms per percent).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

hjr = entry.load_package()
W, H = 1920, 1080
CONFIGS = {"rebuild_opt1": {"device_bvh_opt": 1}, "rebuild_opt0": {"device_bvh_opt": 0},
           "refit_always": {"device_bvh_opt": 1, "device_bvh_refit": 1000, "device_bvh_refit_growth": 10000},
           "refit_default": {"device_bvh_opt": 1, "device_bvh_refit": 1000}}


def motion(arrays, k):
    m0 = np.asarray(arrays["transforms"], dtype=np.float64).reshape(-1, 3, 4)
    n = m0.shape[0]
    m, inv = np.zeros((n, 12), np.float32), np.zeros((n, 12), np.float32)
    for i in range(n):
        a = k * (0.01 + 0.003 * (i % 7))
        mv = np.eye(4)
        mv[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        mv[:3, 3] = 0.02 * k * np.array([(i % 3) - 1.0, ((i % 4) - 1.5) / 1.5, (i % 2) - 0.5])
        full = mv @ np.vstack([m0[i], [0, 0, 0, 1]])
        m[i] = full[:3].reshape(-1).astype(np.float32)
        inv[i] = np.linalg.inv(full)[:3].reshape(-1).astype(np.float32)
    return m, inv


def run(scene, arrays, cam, opt, options, frames):
    d = hjr.Device(0)
    out = []
    try:
        d.set_option("device_bvh", 1)
        d.set_option("force_rebuild", 1)
        for k, v in options.items():
            d.set_option(k, v)
        d.upload_scene(scene.view)
        d.set_transforms(*motion(arrays, 0))  # warm-up: allocations, the scene upload
        d.upload_scene(scene.view)            # ... and frame 0 is a full build in every configuration
        mk = lambda spp, flags=0: hjr.make_params(W, H, spp, cam, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity, flags=flags)  # noqa: E731
        for k in range(frames):
            m, inv = motion(arrays, k)
            t0 = time.perf_counter()
            d.set_transforms(m, inv)
            wall = 1e3 * (time.perf_counter() - t0)
            st = d.stats()
            row = {"frame": k, "build_ms": st["frame_build_ms"], "commit_wall_ms": wall, "bvh_refits": st["bvh_refits"], "bvh_sah": st["bvh_sah"]}
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


def derive(res):
    reb, ref = res["rebuild_opt1"], res["refit_always"]
    build = statistics.median(r["build_ms"] for r in reb[1:])
    refit = statistics.median(r["build_ms"] for r in ref[1:])
    d = {"build_ms_opt1": build, "build_ms_opt0": statistics.median(r["build_ms"] for r in res["rebuild_opt0"][1:]), "refit_ms": refit,
         "build_commit_wall_ms_opt1": statistics.median(r["commit_wall_ms"] for r in reb[1:]),
         "refit_commit_wall_ms": statistics.median(r["commit_wall_ms"] for r in ref[1:])}
    for spp in (64, 8):
        key = "render_ms_%dspp" % spp
        g = np.array([100.0 * (a["bvh_sah"] / b["bvh_sah"] - 1.0) for a, b in zip(ref[1:], reb[1:])])
        dr = np.array([a[key] - b[key] for a, b in zip(ref[1:], reb[1:])])
        slope = float((g * dr).sum() / max((g * g).sum(), 1e-30))
        d["render_ms_per_percent_%dspp" % spp] = slope
        d["break_even_growth_percent_%dspp" % spp] = (build - refit) / slope if slope > 0 else None
    d["sah_growth_percent_last_frame"] = 100.0 * (ref[-1]["bvh_sah"] / reb[-1]["bvh_sah"] - 1.0)
    d["refit_default_full_builds"] = [r["frame"] for r in res["refit_default"] if r["bvh_refits"] == 0]
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_bvh_refit.json"))
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
                     "frames": a.frames}, "configs": {}}
    for name, options in CONFIGS.items():
        res["configs"][name] = run(scene, arrays, cam, opt, options, a.frames)
        print(name, json.dumps(res["configs"][name][-1]), flush=True)
    res["derived"] = derive(res["configs"])
    print("derived", json.dumps(res["derived"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
