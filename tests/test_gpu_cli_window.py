"""The file level of the render window: "Henjou_HIP": {"window": [x0, y0, x1, y1]} and {"bucket": [bw, bh]} through henjou_cli (43 x 29,
16 spp).  A window job writes the window's rows and columns of the whole frame's PNG; a bucketed job writes the unbucketed job's bytes."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from scene_util import ROOT, hjr

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
W, H = 43, 29


def cli_run(tmp_path, name, extra, args=(), spp=16):
    work = tmp_path / "run"
    if not work.exists():
        shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
        shutil.copytree(os.path.join(hjr.ASSETS, "LUT"), work / "LUT")
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Image"].update(image_name=name, image_width=W, image_height=H, max_spp=spp)
    if extra is not None:
        ro["Henjou_HIP"] = extra
    (work / "render_option.json").write_text(json.dumps(ro))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    q = subprocess.run([CLI, "render_option.json"] + list(args), cwd=work, capture_output=True, text=True, timeout=120, env=env)
    assert q.returncode == 0, q.stdout + q.stderr
    path = work / (name + "_001.png")
    return path.read_bytes(), hjr.load_png(str(path)), q.stderr


def test_window_png_is_the_crop_of_the_frame_png(tmp_path):
    """Single process (hjr_render_file), the rank path, and two ranks where the machine has two GPUs: the PNG has the window's size and
    equals rows H - y1 .. H - y0 and columns x0 .. x1 of the whole frame's PNG (the PNG's row 0 is the top)."""
    import torch
    assert os.path.exists(CLI), "henjou_cli is not built"
    _, full, _ = cli_run(tmp_path, "full", None)
    assert full.shape == (H, W, 4)
    for k, win in enumerate(((8, 16, 21, 27), (16, 8, 43, 29))):
        x0, y0, x1, y1 = win
        want = full[H - y1:H - y0, x0:x1]
        runs = [[], ["--rank", "0", "--world", "1"]] + ([["--devices", "2"]] if torch.cuda.device_count() >= 2 else [])
        for j, args in enumerate(runs):
            _, got, _ = cli_run(tmp_path, "win%d_%d" % (k, j), {"window": list(win)}, args)
            assert got.shape == want.shape and np.array_equal(got, want), (win, args)


def test_bucket_png_is_the_unbucketed_png(tmp_path):
    """"bucket": [16, 8] alone, with "passes": 2, with "noise_threshold" (64 spp, so that tiles stop), with firefly_clamp_passes, and
    buckets of a window: byte-identical PNGs."""
    base, _, _ = cli_run(tmp_path, "base", None)
    got, _, err = cli_run(tmp_path, "b", {"bucket": [16, 8]})
    assert "12 buckets" in err, err
    assert got == base
    got, _, err = cli_run(tmp_path, "bp", {"bucket": [16, 8], "passes": 2})
    assert "2 sample passes" in err and "12 buckets" in err, err
    assert got == base
    adaptive = {"noise_threshold": 0.1, "min_samples": 16}
    abase, _, err0 = cli_run(tmp_path, "a", adaptive, spp=64)
    got, _, err = cli_run(tmp_path, "ab", dict(adaptive, bucket=[16, 8]), spp=64)
    assert "adaptive" in err0 and "adaptive" in err, err
    assert got == abase
    assert err0.split("adaptive: ")[1].split(" samples rendered")[0].split()[-1] == err.split("adaptive: ")[1].split(" samples rendered")[0].split()[-1]
    ff = {"firefly_clamp": 4, "firefly_clamp_passes": True, "passes": 4}
    fbase, _, _ = cli_run(tmp_path, "f", ff, spp=64)
    got, _, _ = cli_run(tmp_path, "fb", dict(ff, bucket=[16, 8]), spp=64)
    assert got == fbase
    wbase, _, _ = cli_run(tmp_path, "w", {"window": [8, 8, 43, 27]})
    got, _, err = cli_run(tmp_path, "wb", {"window": [8, 8, 43, 27], "bucket": [16, 8]})
    assert "9 buckets" in err, err
    assert got == wbase
