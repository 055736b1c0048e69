"""tools/deform_bench.py [--out profiles/deform.json] -- the cost of deforming geometry per frame on the 1 M-triangle stress scene
(tools/make_stress_scene.py defaults): K = 4 morph targets with normal deltas over every vertex, device_bvh 1, device_bvh_refit 8.  Run
on the GPU machine from the repository root.

Rows, each the median of 5 commits after a warm-up, the weights changing a little from commit to commit:
  morph_kernel_ms     hjr_morph_kernel alone, HIP events on the context's stream around its launch (the library's verbose line), and the
                      achieved bytes per second against the bytes it streams: (2 + 2 K) x 12 B read + 24 B written per vertex
  commit_morph        set_morph_weights + set_transforms: hjr_stats.frame_build_ms (HIP events around the refit or build) and the wall time
  commit_plain        the same transforms without a morph set, forced ("force_rebuild" 1): what a commit cost before this feature
  commit_update       the same deformation delivered from the host: hjr_update_vertices with the blended positions and normals, then
                      set_transforms (the blend itself, done in numpy ahead of the timed window, is not counted): the path the kernel replaces
A figure that could not be taken is null; nothing here is asserted anywhere.
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

hjr = entry.load_package()
K, REPEATS = 4, 5


class stderr_to_file:
    """the library's verbose lines (C stdio on fd 2) into a file for the length of the block"""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        sys.stderr.flush()
        self.saved = os.dup(2)
        self.f = open(self.path, "w")
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.f.close()
        return False


def weights(step):
    return np.array([0.10 + 0.01 * step, -0.05 + 0.005 * step, 0.02 * step, 0.03], dtype=np.float32)


def blend(base, deltas, w):
    p = base.copy()
    for k in range(len(deltas)):
        p = p + np.float32(w[k]) * deltas[k]
    return p


def commits(d, xf, before, n=REPEATS, warm=1):
    """(frame_build_ms, wall ms, stats) lists of n commits after `warm` untimed ones; before(i) runs ahead of commit i inside the wall time"""
    build, wall, st = [], [], None
    for i in range(warm + n):
        t0 = time.perf_counter()
        before(i)
        d.set_transforms(*xf)
        dt = 1e3 * (time.perf_counter() - t0)
        st = d.stats()
        if i >= warm:
            build.append(st["frame_build_ms"])
            wall.append(dt)
    return build, wall, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform.json"))
    ap.add_argument("--spheres", type=int, default=None, help="make_stress_scene.py --spheres (default: its own, the 1 M-triangle scene)")
    a = ap.parse_args()
    work = tempfile.mkdtemp()
    cmd = [sys.executable, os.path.join(ROOT, "tools", "make_stress_scene.py"), work] + (["--spheres", str(a.spheres)] if a.spheres else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    opt = hjr.load_render_option(os.path.join(work, "render_option_stress.json"))
    scene = hjr.Scene(opt.gltf_path.decode(), opt.gltf_name.decode(), opt)
    arrays = scene.arrays(float(1.0 / opt.fps))
    xf = (arrays["transforms"], arrays["inv_transforms"])
    nv = int(scene.view.n_vertices)
    rng = np.random.default_rng(1)
    base_v, base_n = arrays["vertices"].reshape(-1, 3), arrays["normals"].reshape(-1, 3)
    scale = 0.002 * float((base_v.max(0) - base_v.min(0)).max())  # a deformation that moves a little per frame: refits stay below the growth guard
    pd = (rng.uniform(-1, 1, (K, nv, 3)) * scale).astype(np.float32)
    nd = rng.uniform(-0.05, 0.05, (K, nv, 3)).astype(np.float32)
    sets = [{"first_vertex": 0, "first_weight": 0, "position_deltas": pd, "normal_deltas": nd}]
    streamed = nv * ((2 + 2 * K) * 12 + 24)
    res = {"scene": {"triangles": int(scene.view.n_triangles), "vertices": nv, "instances": int(scene.view.n_instances), "targets": K,
                     "device_bvh": 1, "device_bvh_refit": 8}, "streamed_bytes": streamed}

    def device():
        d = hjr.Device(0)
        d.set_option("device_bvh", 1)
        d.set_option("device_bvh_refit", 8)
        d.upload_scene(scene.view)
        return d

    # without a morph: forced commits of the same transforms
    d = device()
    try:
        d.set_transforms(*xf)
        d.set_option("force_rebuild", 1)
        b, w, st = commits(d, xf, lambda i: None)
        res["commit_plain"] = {"frame_build_ms": statistics.median(b), "wall_ms": statistics.median(w), "all_build_ms": b, "bvh_refits_last": st["bvh_refits"]}
    finally:
        d.close()
    print("commit_plain", json.dumps(res["commit_plain"]), flush=True)

    # with the morph: the weights change per commit
    d = device()
    log = os.path.join(work, "verbose.log")
    try:
        d.set_morph(sets, weights(0))
        d.set_transforms(*xf)
        d.set_option("verbose", 1)
        with stderr_to_file(log):
            b, w, st = commits(d, xf, lambda i: d.set_morph_weights(weights(1 + i)))
        d.set_option("verbose", 0)
        assert st["morph_vertices"] == nv, st
        ms = [float(x) for x in re.findall(r"\[hjr\] morph: \d+ vertices blended on the device, kernel ([0-9.]+) ms", open(log).read())][-REPEATS:]
        k_ms = statistics.median(ms) if ms else None
        res["morph_kernel"] = {"ms": k_ms, "all_ms": ms, "achieved_TB_per_s": streamed / (k_ms * 1e-3) / 1e12 if k_ms else None}
        res["commit_morph"] = {"frame_build_ms": statistics.median(b), "wall_ms": statistics.median(w), "all_build_ms": b, "bvh_refits_last": st["bvh_refits"]}
    finally:
        d.close()
    print("morph_kernel", json.dumps(res["morph_kernel"]), flush=True)
    print("commit_morph", json.dumps(res["commit_morph"]), flush=True)

    # the same deformation from the host
    d = device()
    try:
        d.set_transforms(*xf)
        blended = [(blend(base_v, pd, weights(i)), blend(base_n, nd, weights(i))) for i in range(1 + REPEATS)]
        b, w, st = commits(d, xf, lambda i: d.update_vertices(0, *blended[i]))
        res["commit_update"] = {"frame_build_ms": statistics.median(b), "wall_ms": statistics.median(w), "all_build_ms": b, "bvh_refits_last": st["bvh_refits"],
                                "uploaded_bytes": nv * 24}
    finally:
        d.close()
    print("commit_update", json.dumps(res["commit_update"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
