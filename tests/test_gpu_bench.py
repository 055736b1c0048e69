"""bench.py contract on a GPU: one JSON line with the required keys at N = 1, and a rehearsal of the N = 2 code path
(two ranks pinned to the one GPU of the box, gloo instead of RCCL) — the driver's N = 2/4/8 runs use the same code with nccl."""
import json
import os
import subprocess
import sys

import pytest

from scene_util import ROOT, hjr

pytestmark = pytest.mark.gpu
REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"]
FULL_ONLY = ["color_only", "fast_math", "roofline", "secondary", "cpu_baseline"]


def run(cmd, env=None):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_single_gpu_contract():
    """The plain line carries the headline only; --full adds the measured side blocks to the same keys."""
    cmd = [sys.executable, "bench.py", "--width", "320", "--height", "200", "--spp", "32", "--steps", "2", "--warmup", "1", "--cpu-spp", "2",
           "--stress-spheres", "8", "--stress-segments", "32"]
    plain, d = run(cmd), run(cmd + ["--full"])
    assert not [k for k in FULL_ONLY if k in plain], plain
    for line in (plain, d):
        for k in REQUIRED:
            assert k in line, k
        assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "Msamples/s" and line["dtype"] == "f32"
        assert line["value"] > 0 and line["higher_is_better"] is True and line["vs_baseline"] is None and "workload" in line["config"]
    r = d["roofline"]
    # the bound is chosen from counters collected inside the run: VALU lane-operations for a scene served by LDS / L2
    assert r["counters"]["source"].startswith("rocprofv3"), r["counters"]
    assert (r["bound"], r["peak"], r["unit"]) in (("valu", 157.3, "TFLOP/s"), ("hbm", 8000.0, "GB/s"))
    assert 0 < r["frac"] <= 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic"] > 0 and 0 < r["counters"]["active_lane_frac"] <= 1.0
    assert d["color_only"]["value"] > 0
    big = d["secondary"]["large_scene"]  # the memory-path scene (here a small one) with its measured fabric traffic
    assert "error" not in big, big
    assert big["value"] > 0 and big["triangles"] == 12 + 8 * 960 and big["roofline"]["bound"] == "hbm" and big["roofline"]["traffic"] > 0
    assert 0 < big["roofline"]["frac"] <= 1.0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "Msamples/s"
    assert c["rmse_gpu_vs_cpu"]["value"] < 1e-3 * 50  # 2 spp here: a smoke value; the 1024-spp bar is checked in test_gpu_parity.py


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs DIR: the AOVs of the headline's last timed step as float32 DIR/<name>.npy, equal to a direct render of the same
    frame through the package whatever --steps is; a 1920x1080 frame is cut to the fixed 2^20-pixel sample, under 64 MB in all."""
    import numpy as np
    quick = ["--warmup", "1", "--no-pmc", "--no-cpu-baseline", "--no-secondary"]
    for d, steps in (("a", 1), ("b", 3)):
        r = run([sys.executable, "bench.py", "--width", "320", "--height", "200", "--spp", "8", "--steps", str(steps),
                 "--dump-outputs", str(tmp_path / d)] + quick)
        assert r["steps"] == steps
    cwd = os.getcwd()
    os.chdir(hjr.ASSETS)
    try:
        rd = hjr.Renderer(0)
        rd.loadRenderOption("render_option_c2.json")
        rd.render_option.image_width, rd.render_option.image_height, rd.render_option.max_spp = 320, 200, 8
        rd.render_option.integrator = hjr.INTEGRATOR_NEE
        rd.loadGLTFfile(rd.render_option.gltf_path.decode(), rd.render_option.gltf_name.decode())
        rd.build()
    finally:
        os.chdir(cwd)
    want = dict(zip(("color", "albedo", "normal"), rd.render_frame(rd.render_option.start_frame)))
    assert np.any(want["color"][..., :3] > 0)
    for name, ref in want.items():
        for d in ("a", "b"):
            got = np.load(str(tmp_path / d / (name + ".npy")))
            assert got.dtype == np.float32 and got.shape == (200, 320, 4), (name, got.dtype, got.shape)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (name, d)
    run([sys.executable, "bench.py", "--width", "1920", "--height", "1080", "--spp", "1", "--steps", "1", "--dump-outputs", str(tmp_path / "c")] + quick)
    files = sorted(os.listdir(str(tmp_path / "c")))
    assert files == ["albedo.npy", "color.npy", "normal.npy"]
    assert sum(os.path.getsize(str(tmp_path / "c" / f)) for f in files) <= 64e6
    assert all(np.load(str(tmp_path / "c" / f)).shape == (1 << 20, 4) for f in files)


def test_bench_two_rank_rehearsal():
    env = dict(os.environ, HJR_BENCH_DEVICE="0", HJR_BENCH_BACKEND="gloo")
    d = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
             "--master-port", "29577", "bench.py", "--gpus", "2", "--width", "320", "--height", "200", "--spp", "32", "--steps", "1",
             "--warmup", "1", "--full"], env=env)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0 and "cpu_baseline" not in d
    assert "gather" in d["config"]["parallelism"]


def test_bench_gpus_2_started_plainly_launches_its_own_ranks():
    """`python bench.py --gpus 2` without a launcher: bench.py starts torch.distributed.run itself as a child process and relays rank 0's
    line (rehearsal knobs: both ranks on GPU 0, gloo in place of RCCL — two RCCL ranks need two GPUs)."""
    env = dict(os.environ, HJR_BENCH_DEVICE="0", HJR_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    d = run([sys.executable, "bench.py", "--gpus", "2", "--width", "320", "--height", "200", "--spp", "32", "--steps", "1", "--warmup", "1"], env=env)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    assert "gather" in d["config"]["parallelism"]
