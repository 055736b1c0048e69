"""Host-only parts of the temporal accumulation (hjr_temporal_accumulate, option "denoise_temporal"; csrc/hjr_temporal.hip.h, DESIGN.md
§11.2): the "denoise_temporal" key of the render option and the structs it must not grow, the layout of hjr_gbuffer_px, and the semantics of
the native checker the GPU kernel is compared with (tests/native/temporal_ref.cpp) on synthetic 16 x 12 frames.  No GPU needed.

The synthetic frames: planes facing the camera at depth z (temporal_util.plane_gbuffer), camera f = 2, so a pixel's footprint at distance t is
(2 / 12) * t / 2 = t / 12: 1 / 3 on the wall at z = -4 and 1 / 6 on the object at z = -2.  Reprojected coordinates come out within about
2e-6 of an integer (one ulp of u * H + W, a value in [16, 32)); the second tap of the pair then has a weight of that size, so with previous
colours in [0, 0.25) an output agrees with "lerp against the one previous pixel" within 2e-6 * 0.25 = 5e-7 < 1e-6."""
import ctypes as C
import os
import subprocess

import numpy as np

from scene_util import ROOT, hjr
from temporal_util import MISS, UNKNOWN, identity_xf, plane_gbuffer, temporal_ref, translated, wall_camera
from test_device_bvh import _option_json

f32 = np.float32
W, H = 16, 12
ALPHA = f32(0.2)


def test_render_option_key_and_struct_sizes(tmp_path):
    """"Henjou_HIP": {"denoise_temporal": true} is stored as denoise_variance == 2; "denoise_variance": true alone stays 1; neither
    hjr_render_option nor hjr_params grew (sizes as before this feature: 3224 and 116 bytes), and the ctypes mirrors agree."""
    load = lambda extra: hjr.load_render_option(_option_json(tmp_path, extra))
    assert load({"denoise_temporal": True}).denoise_variance == 2
    assert load({"denoise_temporal": True, "denoise_variance": True}).denoise_variance == 2
    assert load({"denoise_temporal": 1, "denoise_variance": False}).denoise_variance == 2
    assert load({"denoise_variance": True}).denoise_variance == 1
    assert load({"denoise_variance": True, "denoise_temporal": False}).denoise_variance == 1
    for extra in (None, {"seed": 3}, {"denoise_temporal": False}, {"denoise_temporal": 0}):
        assert load(extra).denoise_variance == 0
    src = tmp_path / "off.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "henjou_hip.h"
#define O(f) offsetof(hjr_gbuffer_px, f)
#define T(f) offsetof(hjr_temporal_frame, f)
int main(void) {
    printf("%zu %zu\\n", sizeof(hjr_render_option), sizeof(hjr_params));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", O(prim), O(inst), O(t), O(b1), O(b2), O(pos), O(ng), O(pad), sizeof(hjr_gbuffer_px));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", T(width), T(height), T(n_instances), T(camera), T(transforms12), T(inv_transforms12), T(gbuffer), T(color),
           T(variance), T(history), sizeof(hjr_temporal_frame));
    printf("%.9g\\n", (double)HJR_TEMPORAL_ALPHA);
    return 0;
}
""")
    exe = str(tmp_path / "off")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = [l.split() for l in subprocess.check_output([exe]).decode().splitlines()]
    assert list(map(int, lines[0])) == [3224, 116] == [C.sizeof(hjr.RenderOption), C.sizeof(hjr.ParamsV2)]
    assert hjr.RenderOption.denoise_variance.offset + 4 == C.sizeof(hjr.RenderOption), "denoise_variance is still the last field"
    D = hjr.GBUFFER_DTYPE
    assert list(map(int, lines[1])) == [D.fields[n][1] for n in ("prim", "inst", "t", "b1", "b2", "pos", "ng", "pad")] + [D.itemsize] and D.itemsize == 48
    F = hjr.TemporalFrame
    assert list(map(int, lines[2])) == [getattr(F, n).offset for n in ("width", "height", "n_instances", "camera", "transforms12", "inv_transforms12", "gbuffer", "color",
                                                                         "variance", "history")] + [C.sizeof(F)]
    assert f32(float(lines[3][0])) == hjr.TEMPORAL_ALPHA == ALPHA


def frame(cam, planes, xf=None, seed=0, hist=None, n_inst=2):
    """A synthetic frame: colours in [0, 0.25), alpha a ramp, variances in [0.01, 0.02)."""
    rng = np.random.default_rng(seed)
    m, inv = xf if xf is not None else (identity_xf(n_inst), identity_xf(n_inst))
    color = rng.uniform(0, 0.25, (H, W, 4)).astype(f32)
    color[..., 3] = np.linspace(0, 1, H * W, dtype=f32).reshape(H, W) + f32(seed)
    d = {"camera": cam, "transforms": m, "inv_transforms": inv, "gbuffer": plane_gbuffer(W, H, cam, planes), "color": color,
         "variance": rng.uniform(0.01, 0.02, (H, W)).astype(f32)}
    if hist is not None:
        d["history"] = np.full((H, W), hist, f32)
    return d


WALL = (-4.0, 0, 7, -1e9, 1e9)


def lerp(prev_rgb, cur_rgb, alpha):
    return prev_rgb + (cur_rgb - prev_rgb) * alpha


def test_identity():
    """A fronto-parallel wall, identical cameras: every pixel finds its own history."""
    cam = wall_camera()
    for hist, alpha, h_out in ((2.0, f32(1) / f32(3), 3.0), (9.0, ALPHA, 10.0), (64.0, ALPHA, 64.0)):
        prev, cur = frame(cam, [WALL], seed=1, hist=hist), frame(cam, [WALL], seed=2)
        c, v, h = temporal_ref(prev, cur, 12)
        assert np.abs(h - f32(h_out)).max() <= 1e-5, "h = min(h_prev + 1, 64)"
        assert np.abs(c[..., :3] - lerp(prev["color"][..., :3], cur["color"][..., :3], alpha)).max() <= 1e-6
        assert np.array_equal(c[..., 3], cur["color"][..., 3]), "alpha is the current frame's"
        want_v = (1 - float(alpha)) ** 2 * prev["variance"].astype(np.float64) + float(alpha) ** 2 * cur["variance"]
        assert np.abs(v - want_v).max() <= 1e-7
    c, v, h = temporal_ref(None, cur, 12)
    assert np.array_equal(c, cur["color"]) and np.array_equal(v, cur["variance"]) and (h == 1).all(), "no previous frame: restart"


def test_camera_moved_by_three_pixel_footprints():
    """The camera moves by 3 footprints (1.0 on the wall at distance 4) to +x: the current pixel x shows what the previous pixel x + 3
    showed; the three rightmost columns have no source and restart."""
    prev, cur = frame(wall_camera(0.0), [WALL], seed=3, hist=5.0), frame(wall_camera(1.0), [WALL], seed=4)
    c, v, h = temporal_ref(prev, cur, 12)
    assert np.abs(c[:, :W - 3, :3] - lerp(prev["color"][:, 3:, :3], cur["color"][:, :W - 3, :3], ALPHA)).max() <= 1e-5
    assert np.abs(h[:, :W - 3] - 6).max() <= 1e-5
    assert np.array_equal(c[:, W - 3:], cur["color"][:, W - 3:]) and np.array_equal(v[:, W - 3:], cur["variance"][:, W - 3:]) and (h[:, W - 3:] == 1).all()
    # and in y: 2 footprints up (world y + 2/3): previous row y + 2
    cur = frame(wall_camera(0.0, 2.0 / 3.0), [WALL], seed=4)
    c, v, h = temporal_ref(prev, cur, 12)
    assert np.abs(c[:H - 2, :, :3] - lerp(prev["color"][2:, :, :3], cur["color"][:H - 2, :, :3], ALPHA)).max() <= 1e-5
    assert (h[H - 2:] == 1).all() and np.abs(h[:H - 2] - 6).max() <= 1e-5


def test_moving_object_disoccludes_and_is_followed():
    """Instance 1, a strip at z = -2 over world x in [-0.5, 0.5) (pixels 5..10), moves by +0.5 = 3 of its footprints (pixels 8..13).  Its pixels
    take their history from where it was; the wall pixels it uncovers (5..7) restart: 6 and 7 surely (both taps of either pair showed the
    object), 5 unless its left neighbour, a wall pixel, enters with its weight of about 1e-6."""
    cam = wall_camera()
    xf_prev = (identity_xf(2), identity_xf(2))
    m, inv = translated(identity_xf(2)[1:], identity_xf(2)[1:], (0.5, 0, 0))
    xf_cur = (np.concatenate([identity_xf(1), m]), np.concatenate([identity_xf(1), inv]))
    prev = frame(cam, [WALL, (-2.0, 1, 3, -0.5, 0.5)], xf_prev, seed=5, hist=7.0)
    cur = frame(cam, [WALL, (-2.0, 1, 3, 0.0, 1.0)], xf_cur, seed=6)
    assert (prev["gbuffer"]["inst"][0] == [0] * 5 + [1] * 6 + [0] * 5).all() and (cur["gbuffer"]["inst"][0] == [0] * 8 + [1] * 6 + [0] * 2).all()
    c, v, h = temporal_ref(prev, cur, 12)
    assert (h[:, 6:8] == 1).all() and np.array_equal(c[:, 6:8], cur["color"][:, 6:8]), "uncovered wall pixels restart"
    assert np.abs(h[:, 8:14] - 8).max() <= 1e-5, "the object's pixels keep their history"
    assert np.abs(c[:, 8:14, :3] - lerp(prev["color"][:, 5:11, :3], cur["color"][:, 8:14, :3], ALPHA)).max() <= 1e-5, "... from where the object was"
    assert np.abs(h[:, :5] - 8).max() <= 1e-5 and np.abs(h[:, 14:] - 8).max() <= 1e-5, "the static wall keeps its history"
    # the wall 2 units behind a tap of the object fails the plane test even with matching ids
    same = dict(prev)
    same["gbuffer"] = prev["gbuffer"].copy()
    same["gbuffer"]["inst"] = 0
    cur0 = frame(cam, [WALL], seed=6)
    _, _, h = temporal_ref(same, cur0, 12)
    assert (h[:, 6:10] == 1).all(), "a tap on another surface is refused by the plane distance"


def test_mismatched_instance_ids_invalidate():
    cam = wall_camera()
    prev, cur = frame(cam, [WALL], seed=7, hist=3.0), frame(cam, [WALL], seed=8)
    prev["gbuffer"]["inst"] = 1
    c, v, h = temporal_ref(prev, cur, 12)
    assert (h == 1).all() and np.array_equal(c, cur["color"]) and np.array_equal(v, cur["variance"])


def _near(mask):
    """mask dilated by one pixel (the tap pair of a pixel may reach one neighbour with a weight near 0)."""
    m = mask.copy()
    m[1:] |= mask[:-1]; m[:-1] |= mask[1:]
    n = m.copy()
    n[:, 1:] |= m[:, :-1]; n[:, :-1] |= m[:, 1:]
    return n


def test_unknown_nan_and_negative_variances():
    cam = wall_camera()
    prev, cur = frame(cam, [WALL], seed=9, hist=4.0), frame(cam, [WALL], seed=10)
    bad = np.zeros((H, W), bool)
    prev["variance"][2, 3] = UNKNOWN; prev["variance"][5, 9] = np.nan; prev["variance"][10, 1] = np.inf
    cur["variance"][7, 12] = UNKNOWN; cur["variance"][0, 0] = np.nan; cur["variance"][11, 15] = f32(2e30)
    for y, x in ((2, 3), (5, 9), (10, 1), (7, 12), (0, 0), (11, 15)):
        bad[y, x] = True
    c, v, h = temporal_ref(prev, cur, 12)
    assert (v[bad] == UNKNOWN).all(), "UNKNOWN, NaN, inf and values above UNKNOWN give UNKNOWN"
    far = ~_near(bad)
    assert np.isfinite(v[far]).all() and (v[far] < 0.02).all() and (v[far] > 0).all()
    assert np.isfinite(c).all() and np.abs(h - 5).max() <= 1e-5, "colour and history are not affected"
    # negative variances act as 0, on either side
    neg_p, neg_c, zero_p, zero_c = dict(prev), dict(cur), dict(prev), dict(cur)
    for d, val in ((neg_p, -1.0), (zero_p, 0.0), (neg_c, -np.inf), (zero_c, 0.0)):
        d["variance"] = frame(cam, [WALL], seed=11)["variance"]
        d["variance"][3:6, 4:8] = val
    a, b = temporal_ref(neg_p, neg_c, 12), temporal_ref(zero_p, zero_c, 12)
    assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b))
    assert (a[1] >= 0).all()


def hostile(d, prev_side):
    """Poisons records of a frame in place: prim / inst out of range, non-finite and huge positions and normals.  Returns the mask."""
    g = d["gbuffer"]
    bad = np.zeros(g.shape, bool)
    g["prim"][1, 2] = 12; g["prim"][1, 3] = 0xfffffffe; g["inst"][2, 5] = 2; g["inst"][2, 6] = 0xffffffff; g["inst"][2, 7] = 0x80000000
    g["pos"][4, 4] = np.nan; g["pos"][4, 5] = [np.inf, 0, -4]; g["pos"][4, 6] = [0, -np.inf, np.nan]; g["pos"][4, 7] = [3e38, 3e38, -3e38]
    g["ng"][6, 8] = np.nan; g["ng"][6, 9] = np.inf; g["ng"][6, 10] = 0
    g["pos"][8, 1] = [0, 0, 4]   # behind the camera
    g["pos"][8, 2] = [0, 0, 0]   # at the camera
    for y, x in ((1, 2), (1, 3), (2, 5), (2, 6), (2, 7), (4, 4), (4, 5), (4, 6), (4, 7), (6, 8), (6, 9), (8, 1), (8, 2)):
        bad[y, x] = True
    if prev_side:
        d["history"][10, 9] = np.nan; d["history"][10, 12] = -np.inf; d["history"][3, 13] = np.inf
        bad[10, 9] = bad[10, 12] = bad[3, 13] = True
    return bad


def test_hostile_records_restart_and_stay_finite():
    """prim / inst out of range and non-finite positions in the current frame restart the pixel; in the previous frame they are invalid
    taps; and nothing non-finite reaches an output."""
    cam = wall_camera()
    prev, cur = frame(cam, [WALL], seed=12, hist=6.0), frame(cam, [WALL], seed=13)
    bad = hostile(cur, False)
    c, v, h = temporal_ref(prev, cur, 12)
    assert np.isfinite(c).all() and np.isfinite(v).all() and np.isfinite(h).all()
    restart = bad.copy()
    restart[6, 10] = False  # ng = 0: both limits are 0 and so are both left sides: the comparisons hold (0 <= 0)
    assert (h[restart] == 1).all() and np.array_equal(c[restart], cur["color"][restart])
    assert np.abs(h[~bad] - 7).max() <= 1e-5
    prev, cur = frame(cam, [WALL], seed=12, hist=6.0), frame(cam, [WALL], seed=13)
    bad = hostile(prev, True)
    c, v, h = temporal_ref(prev, cur, 12)
    assert np.isfinite(c).all() and np.isfinite(v).all() and np.isfinite(h).all() and (h >= 1).all() and (h <= 64).all()
    far = ~_near(bad)
    assert np.abs(h[far] - 7).max() <= 1e-5
    assert (h[10, 9] == 1) and (h[10, 12] == 1) and (h[3, 13] == 64), "a NaN or negative history restarts the count, an infinite one saturates"
