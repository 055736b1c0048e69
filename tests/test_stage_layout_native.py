"""Host test (CPU) of the staging arena of the host-buffer entry points (henjou-renderer_amd/host/stage_layout.hpp, used by HostStage in
csrc/hjr_device_internal.h): tests/native/stage_layout_test.cpp, a stand-alone program built with AddressSanitizer and UBSan, lays out mixed
alignments, zero-byte items, a single item and the item list of hjr_temporal_accumulate_response at 7 x 5 pixels with 3 instances, and
checks that every offset is a multiple of its alignment, that no two items overlap and that the total covers the last item."""
import os
import subprocess

from scene_util import ROOT


def test_stage_layout_native(tmp_path):
    exe = str(tmp_path / "stage_layout_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "native", "stage_layout_test.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "stage_layout_test ok" in p.stdout
