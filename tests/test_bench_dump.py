"""bench.py --dump-outputs, host side (no GPU): file names and dtype, the whole frame while it fits, otherwise the same seeded
2^20-pixel sample in every file, under 64 MB for three full-HD AOVs and identical from run to run."""
import os

import numpy as np
import torch

import bench


def test_small_frame_is_written_whole(tmp_path):
    t = torch.rand(200, 320, 4, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path), {"color": t})
    assert os.listdir(str(tmp_path)) == ["color.npy"]
    a = np.load(str(tmp_path / "color.npy"))
    assert a.dtype == np.float32 and np.array_equal(a, t.numpy())


def test_full_hd_frame_is_one_fixed_sample(tmp_path):
    aovs = {k: torch.rand(1080, 1920, 4, dtype=torch.float32) for k in ("color", "albedo", "normal")}
    bench.dump_outputs(str(tmp_path / "a"), aovs)
    bench.dump_outputs(str(tmp_path / "b"), aovs)
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == ["albedo.npy", "color.npy", "normal.npy"]
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in files) <= 64e6
    pick = np.sort(np.random.default_rng(0).choice(1080 * 1920, bench.DUMP_SAMPLE_PIXELS, replace=False))
    for name, t in aovs.items():
        a = np.load(str(tmp_path / "a" / (name + ".npy")))
        assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE_PIXELS, 4)
        assert np.array_equal(a, t.reshape(-1, 4).numpy()[pick])
        assert np.array_equal(a, np.load(str(tmp_path / "b" / (name + ".npy"))))
