"""Host test (CPU) of the megakernel's work-item arithmetic (csrc/hjr_layout.h): tests/native/item_decode_test.cpp walks the queue the way
the kernel does — 64 aligned items per wave, one item per lane, chunk after chunk until the item's last — and checks that every (owned
tile, chunk, pixel) of a launch is rendered exactly once for every group length, shard, sample pass and tile list."""
import os
import subprocess

from scene_util import ROOT


def test_item_decode_native(tmp_path):
    exe = str(tmp_path / "item_decode_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "native", "item_decode_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "item_decode_test ok" in p.stdout
