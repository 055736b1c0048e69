"""tools/device_bvh_instances_bench.py [--out profiles/device_bvh_instances.json] [--frames 16] -- per-instance trees under a per-commit top
tree (option "device_bvh_instances") against a full device build every frame and against refitting, on the scene and the 16-frame
motion of tools/device_bvh_refit_bench.py (1 M-triangle stress scene, 1920x1080 NEE at 64 and at 8 spp).  Run on the GPU machine from
the repository root.

Configurations, all in this process on the same transforms (device_bvh 1, device_bvh_opt 1):
  rebuild        a full build every frame
  refit_default  device_bvh_refit 1000 with the default growth guard
  instances      device_bvh_instances 1: the topology once (bvh_topology_ms), flatten + boxes + top tree + collapse every frame
  graft          ... plus device_bvh_graft 1: the instances' BVH4s once as well; flatten + node boxes + top tree + placement every frame
With --repeat N (default 2) the two instance configurations run N times, alternating (instances / graft / instances_2 / graft_2): the
spread between equal runs is the noise the graft's margin over the instance trees is compared with (derived "graft_margin").
With --commits N [--config graft] nothing is rendered or written: one topology build and N commits of that configuration, for a run under
rocprofv3 --kernel-trace --stats (profiles/device_bvh_graft_kernel_stats.csv; a run of its own, no counters with it).
Per frame: hjr_stats.frame_build_ms (the commit's kernels, HIP-event time) and the wall time of hjr_set_transforms, bvh_topology_ms,
bvh_instances, bvh_refits, bvh_sah, the render kernel time at 64 and at 8 spp (median of 3 launches), node steps per closest ray.
Derived per configuration: commit + render over the frames at 64 and at 8 spp, bvh_sah at frames 0, 7 and 15, node steps at the last frame,
the bytes of topology kept between commits (from the array sizes in csrc/hjr_bvh_build.hip; the skeleton counted as all bvh_nodes nodes).
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
CONFIGS = {"rebuild": {}, "refit_default": {"device_bvh_refit": 1000}, "instances": {"device_bvh_instances": 1},
           "graft": {"device_bvh_instances": 1, "device_bvh_graft": 1}}


def kept_bytes(name, n_tris, n_inst, n_nodes):
    """device memory of the topology a configuration keeps between commits"""
    if name.startswith("instances"):  # child, range 8 + 8, parent 2 x 4, pos, order, top 3 x 4 per triangle; top_ids, root, list per instance
        return 36 * n_tris + 12 * n_inst
    if name.startswith("graft"):      # pos, order per triangle; refs row 16 + parent 4 per skeleton node; list, inst_ref, inst_stat, top_box per instance
        return 8 * n_tris + 20 * n_nodes + (4 + 4 + 8 + 64) * n_inst
    return 0


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
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--commits", type=int, default=0)
    ap.add_argument("--config", default="graft", choices=sorted(CONFIGS))
    a = ap.parse_args()
    work = tempfile.mkdtemp()
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_stress_scene.py"), work], stdout=subprocess.DEVNULL)
    opt = hjr.load_render_option(os.path.join(work, "render_option_stress.json"))
    scene = hjr.Scene(opt.gltf_path.decode(), opt.gltf_name.decode(), opt)
    t = float(1.0 / opt.fps)
    arrays = scene.arrays(t)
    cam = scene.camera(opt, t)
    if a.commits:
        d = hjr.Device(0)
        try:
            for k, v in dict({"device_bvh": 1, "device_bvh_opt": 1, "force_rebuild": 1}, **CONFIGS[a.config]).items():
                d.set_option(k, v)
            d.upload_scene(scene.view)
            for k in range(a.commits):
                d.set_transforms(*rb.motion(arrays, k))
            print(a.config, json.dumps({k: v for k, v in d.stats().items() if k.startswith("bvh_") or k == "frame_build_ms"}))
        finally:
            d.close()
        return
    res = {"scene": {"triangles": int(scene.view.n_triangles), "instances": int(scene.view.n_instances), "width": W, "height": H, "integrator": "NEE",
                     "frames": a.frames}, "configs": {}, "derived": {}}
    order = ["rebuild", "refit_default"] + [n + ("_%d" % (r + 1) if r else "") for r in range(max(a.repeat, 1)) for n in ("instances", "graft")]
    for name in order:
        rows = res["configs"][name] = run(scene, arrays, cam, opt, CONFIGS[name.split("_")[0] if name[-1].isdigit() else name], a.frames)
        res["derived"][name] = derive(rows)
        res["derived"][name]["kept_topology_bytes"] = kept_bytes(name, int(scene.view.n_triangles), rows[-1]["bvh_instances"], rows[-1]["bvh_nodes"])
        print(name, json.dumps(res["derived"][name]), flush=True)
    if a.repeat >= 2:  # the graft's margin: both of its medians below both of the instance trees', by more than equal runs differ
        med = lambda n: [res["derived"][k]["commit_ms_median"] for k in order if k.split("_")[0] == n and k != "refit_default"]  # noqa: E731
        mi, mg = med("instances"), med("graft")
        spread = max(max(mi) - min(mi), max(mg) - min(mg))
        res["derived"]["graft_margin"] = {"instances_commit_ms_median": mi, "graft_commit_ms_median": mg, "spread_between_equal_runs_ms": spread,
                                          "margin_ms": min(mi) - max(mg), "holds": min(mi) - max(mg) > spread}
        print("graft_margin", json.dumps(res["derived"]["graft_margin"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
