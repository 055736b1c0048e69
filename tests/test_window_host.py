"""Host side of the render window (include/henjou_hip.h: hjr_params_window.window): bucket helpers, hjr_blit_window, the "window" / "bucket" keys
of the "Henjou_HIP" section and the refusals of the file drivers.  No GPU: the drivers refuse before a scene is loaded or a device touched.
The host code new to the feature also runs under ASan / UBSan as a stand-alone program (tests/native/window_test.cpp)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from scene_util import ROOT, hjr
from test_device_bvh import _option_json

ERR_ARG = -1
CLI = os.path.join(hjr.PKG_DIR, "henjou_cli")


@pytest.mark.parametrize("w,h,bw,bh", [(43, 29, 16, 8), (43, 29, 8, 8), (43, 29, 48, 32), (8, 8, 8, 8)])
def test_buckets_cover_every_pixel_once(w, h, bw, bh):
    wins = hjr.bucket_windows(w, h, bw, bh)
    assert len(wins) == hjr.lib().hjr_bucket_count(w, h, bw, bh) == -(-w // bw) * -(-h // bh)
    cover = np.zeros((h, w), np.int32)
    for x0, y0, x1, y1 in wins:
        assert x0 % 8 == 0 and y0 % 8 == 0 and x0 < x1 <= w and y0 < y1 <= h and x1 - x0 <= bw and y1 - y0 <= bh
        cover[y0:y1, x0:x1] += 1
    assert (cover == 1).all()
    assert wins == sorted(wins, key=lambda r: (r[1], r[0])), "buckets run row-major"
    out = (C.c_uint32 * 4)(7, 7, 7, 7)
    assert hjr.lib().hjr_bucket_window(w, h, bw, bh, len(wins), out) == ERR_ARG and b"index" in hjr.lib().hjr_last_error()
    assert list(out) == [7, 7, 7, 7]


def test_bucket_sides_must_be_multiples_of_8():
    L = hjr.lib()
    out = (C.c_uint32 * 4)()
    for bw, bh in ((12, 8), (16, 4), (0, 8), (16, 0)):
        assert L.hjr_bucket_count(43, 29, bw, bh) == 0
        assert L.hjr_bucket_window(43, 29, bw, bh, 0, out) == ERR_ARG and b"multiples of 8" in L.hjr_last_error()
        with pytest.raises(hjr.HjrError, match="multiples of 8"):
            hjr.bucket_windows(43, 29, bw, bh)


def test_blit_window_equals_numpy_slicing():
    rng = np.random.default_rng(5)
    w, h = 43, 29
    for win in ((8, 8, 32, 24), (0, 0, 8, 8), (8, 16, 21, 27), (16, 8, 43, 29), (0, 0, 43, 29), (3, 5, 4, 6)):
        x0, y0, x1, y1 = win
        img = rng.random((y1 - y0, x1 - x0, 4), dtype=np.float32)
        frame = rng.random((h, w, 4), dtype=np.float32)
        want = frame.copy()
        want[y0:y1, x0:x1] = img
        assert hjr.blit_window(img, win, frame) is frame and (frame.view(np.uint32) == want.view(np.uint32)).all()
    frame = np.zeros((h, w, 4), np.float32)
    for bad in ((8, 8, 44, 24), (8, 8, 32, 30), (8, 8, 8, 24), (8, 24, 32, 24)):
        img = np.zeros((max(bad[3] - bad[1], 0), max(bad[2] - bad[0], 0), 4), np.float32)
        assert hjr.lib().hjr_blit_window(img.ctypes.data if img.size else frame.ctypes.data, (C.c_uint32 * 4)(*bad), frame.ctypes.data, w, h) == ERR_ARG
        assert b"window" in hjr.lib().hjr_last_error()
    assert not frame.any()


def test_python_mirrors_of_the_window_fields(tmp_path):
    """ParamsV3 / RenderOptionV2 mirror hjr_params_window / hjr_render_option_window: the window fields right behind ParamsV2 / RenderOption,
    which keep the sizes of hjr_params / hjr_render_option."""
    src = tmp_path / "off.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "henjou_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(hjr_params, sample_end), offsetof(hjr_params_window, window), sizeof(hjr_params_window),
           offsetof(hjr_render_option_window, window), offsetof(hjr_render_option_window, bucket), sizeof(hjr_render_option_window));
    return 0;
}
""")
    exe = str(tmp_path / "off")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    se, pw, ps, ow, ob_, os_ = map(int, subprocess.check_output([exe]).split())
    assert pw == se + 4 == C.sizeof(hjr.ParamsV2) == hjr.ParamsV3.window.offset and ps == pw + 16 == C.sizeof(hjr.ParamsV3)
    assert ow == C.sizeof(hjr.RenderOption) == hjr.RenderOptionV2.window.offset and ob_ == ow + 16 == hjr.RenderOptionV2.bucket.offset
    assert os_ == ob_ + 8 == C.sizeof(hjr.RenderOptionV2)
    cam = {"pos": [0, 0, 0], "dir": [0, 0, 1], "up": [0, 1, 0], "right": [1, 0, 0], "f": 1.0}
    p = hjr.make_params(43, 29, 16, cam)
    assert type(p) is hjr.ParamsV2 and p.struct_size == pw and hjr.window_shape(p) == (29, 43)  # without a window: the caller it always was
    p = hjr.make_params(43, 29, 16, cam, window=(8, 16, 21, 27))
    assert isinstance(p, hjr.ParamsV3) and p.struct_size == ps and list(p.window) == [8, 16, 21, 27] and hjr.window_shape(p) == (11, 13)
    assert hjr.window_shape(hjr.ParamsV3()) == (0, 0)


def test_loader_round_trips_window_and_bucket(tmp_path):
    o = hjr.load_render_option(_option_json(tmp_path, {"window": [8, 16, 24, 27], "bucket": [16, 8]}))
    assert isinstance(o, hjr.RenderOptionV2) and list(o.window) == [8, 16, 24, 27] and list(o.bucket) == [16, 8]
    for extra in (None, {"seed": 3}, {"passes": 4}):
        o = hjr.load_render_option(_option_json(tmp_path, extra))
        assert list(o.window) == [0, 0, 0, 0] and list(o.bucket) == [0, 0]
    o = hjr.load_render_option(_option_json(tmp_path, {"window": [0, 0, 8192, 8192], "bucket": [8192, 8]}))
    assert list(o.window) == [0, 0, 8192, 8192] and list(o.bucket) == [8192, 8]


@pytest.mark.parametrize("key,bad", [("window", [8, 8, 32]), ("window", [8, 8, 32, 24, 1]), ("window", 8), ("window", [-8, 8, 32, 24]),
                                      ("window", [8, 8, 32.5, 24]), ("window", [4, 8, 32, 24]), ("window", [8, 12, 32, 24]),
                                      ("window", [32, 8, 32, 24]), ("window", [8, 24, 32, 8]), ("window", [8, 8, "32", 24]),
                                      ("window", [8, 8, 8200, 24]),
                                      ("bucket", [16]), ("bucket", [16, 8, 8]), ("bucket", [-16, 8]), ("bucket", [16.5, 8]),
                                      ("bucket", [12, 8]), ("bucket", [16, 0]), ("bucket", "16x8"), ("bucket", [16, 8200])])
def test_loader_rejects_malformed_values(tmp_path, key, bad):
    with pytest.raises(hjr.HjrError, match="Henjou_HIP." + key):
        hjr.load_render_option(_option_json(tmp_path, {key: bad}))


def test_a_bad_window_is_reported_after_every_older_key(tmp_path):
    """The two keys are read behind every other key of the section: a file that was an error stays that error, and with the older key
    mended the same file reports the window key."""
    with pytest.raises(hjr.HjrError, match="Henjou_HIP.passes"):
        hjr.load_render_option(_option_json(tmp_path, {"window": [4, 8, 32, 24], "passes": 0}))
    with pytest.raises(hjr.HjrError, match="Henjou_HIP.window"):
        hjr.load_render_option(_option_json(tmp_path, {"window": [4, 8, 32, 24], "passes": 2}))
    with pytest.raises(hjr.HjrError, match="Henjou_HIP.min_samples"):
        hjr.load_render_option(_option_json(tmp_path, {"bucket": [12, 8], "min_samples": -1}))
    with pytest.raises(hjr.HjrError, match="Henjou_HIP.bucket"):
        hjr.load_render_option(_option_json(tmp_path, {"bucket": [12, 8], "min_samples": 16}))


def job_json(tmp_path, section, mode="Default", name="x.json"):
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["GLTF_file"]["gltf_filepath"] = str(tmp_path / "no_such_scene") + "/"
    ro["Render_mode"] = mode
    ro["Image"]["image_width"], ro["Image"]["image_height"] = 43, 29
    ro["Henjou_HIP"] = section
    p = tmp_path / name
    p.write_text(json.dumps(ro))
    return p


REFUSALS = [
    ({"window": [8, 8, 32, 24]}, "Denoise", '"window" and "bucket" need Render_mode Default: the Denoise modes filter whole frames'),
    ({"bucket": [16, 8]}, "DenoiseUpScale2X", '"window" and "bucket" need Render_mode Default: the Denoise modes filter whole frames'),
    ({"window": [8, 8, 44, 24]}, "Default", '"window" reaches outside the 43 x 29 image'),
    ({"window": [8, 8, 32, 30]}, "Default", '"window" reaches outside the 43 x 29 image'),
]


@pytest.mark.parametrize("section,mode,text", REFUSALS)
def test_file_drivers_refuse(tmp_path, section, mode, text):
    """hjr_render_file and a rank of henjou_cli give job_check's text before the scene (which does not exist) is loaded."""
    path = job_json(tmp_path, section, mode)
    assert hjr.lib().hjr_render_file(os.fsencode(str(path)), 0) == ERR_ARG
    assert hjr.lib().hjr_last_error().decode() == "hjr_render_file: " + text
    p = subprocess.run([CLI, str(path), "--rank", "0", "--world", "1"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 1 and p.stderr.splitlines() == ["henjou_cli: " + text]


def test_adaptive_temporal_refuses_window_and_bucket(tmp_path):
    text = '"adaptive_temporal" cannot be combined with "window" or "bucket": its prior is gathered over the whole frame'
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["GLTF_file"]["gltf_filepath"] = str(tmp_path / "no_such_scene") + "/"
    for extra in ({"window": [8, 8, 32, 24]}, {"bucket": [16, 8]}):
        # (the Denoise refusal comes first in a Denoise mode, where the key acts; in Default mode the key is stored and refused with these)
        ro["Henjou_HIP"] = dict({"denoise_temporal": True, "adaptive_temporal": True}, **extra)
        path = tmp_path / "at.json"
        path.write_text(json.dumps(ro))
        assert hjr.lib().hjr_render_file(os.fsencode(str(path)), 0) == ERR_ARG
        assert hjr.lib().hjr_last_error().decode() == "hjr_render_file: " + text


def test_cli_refuses_bucket_with_several_devices(tmp_path):
    want = 'henjou_cli: "bucket" cannot be combined with "devices" > 1: buckets are composed on the one device that renders them'
    path = job_json(tmp_path, {"bucket": [16, 8]})
    path2 = job_json(tmp_path, {"bucket": [16, 8], "devices": 2}, name="y.json")
    for cmd in ([CLI, str(path), "--devices", "2"], [CLI, str(path), "--rank", "1", "--world", "2", "--id-fd", "0"], [CLI, str(path2)]):
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=60, cwd=tmp_path, stdin=subprocess.DEVNULL)
        assert p.returncode == 1 and p.stderr.splitlines() == [want], (cmd, p.stderr[-800:])
    # a window alone may be sharded, and one device takes buckets: both go on to the scene file, which does not exist
    for cmd in ([CLI, str(job_json(tmp_path, {"window": [8, 8, 32, 24]}, name="z.json")), "--rank", "1", "--world", "2", "--id-fd", "0"],
                [CLI, str(path), "--devices", "1"]):
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=60, cwd=tmp_path, stdin=subprocess.DEVNULL)
        assert p.returncode == 1 and "cannot be combined" not in p.stderr and "no_such_scene" in p.stderr, (cmd, p.stderr[-800:])


def test_window_host_code_under_asan_ubsan(tmp_path):
    """tests/native/window_test.cpp with the host sources, -fsanitize=address,undefined: bucket helpers, hjr_blit_window, and the two keys
    into callers with the short and a longer hjr_render_option, every buffer exactly as large as its caller says."""
    exe = str(tmp_path / "window_test")
    host = os.path.join(ROOT, "henjou-renderer_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "native", "window_test.cpp"), os.path.join(host, "capi.cpp"), os.path.join(host, "loaders.cpp"),
                           os.path.join(host, "image_io.cpp"), os.path.join(host, "jpeg.cpp"), "-o", exe, "-lz", "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, _option_json(tmp_path, {"window": [8, 16, 24, 27], "bucket": [16, 8]})], capture_output=True, text=True, env=env, timeout=300,
                       cwd=hjr.ASSETS)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    assert "window_test ok" in p.stdout
