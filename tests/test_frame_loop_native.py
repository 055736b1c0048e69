"""The frame loop of the two drivers (henjou-renderer_amd/host/frame_loop.hpp) without a GPU: tests/native/frame_loop_test.cpp
drives render_passes, FrameWriter and ScenePrefetch with fakes.  One program, built three ways, each its own executable and run directly: plain,
with the address and undefined-behaviour sanitizers, and with the thread sanitizer (the two threads of the loop never ran under one: inside
hjr_render_file they touch the device in almost every line)."""
import os
import subprocess

import pytest

from scene_util import ROOT

SOURCE = os.path.join(ROOT, "tests", "native", "frame_loop_test.cpp")
BUILDS = {
    "plain": [],
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
    "tsan": ["-fsanitize=thread"],
}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_frame_loop_native(tmp_path, build):
    out = str(tmp_path / ("frame_loop_test_" + build))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread"] + BUILDS[build] + [SOURCE, "-o", out])
    p = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "frame_loop_test ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
