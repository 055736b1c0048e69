"""Host-only parts of the coverage-aware temporal accumulation (hjr_temporal_frame.coverage, option "denoise_temporal_coverage";
csrc/hjr_temporal.hip.h): the native checker the GPU kernels are compared with (tests/native/temporal_cov_ref.cpp) on
hand-made records, one case per clause of rules 2' and 3'; its equality with tests/native/temporal_ref.cpp when neither side carries
coverage; the option table and the file key.  No GPU needed.

The synthetic frames are tests/test_temporal_host.py's: a wall at z = -4 facing a camera with f = 2 at 16 x 12, so a pixel's footprint on
the wall is 1 / 3 and a camera shift of s / 3 in x (or y) moves every reprojected position by s pixels: xp = x + s up to a few 1e-6."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from scene_util import ROOT, hjr
from temporal_cov_util import SNAP, gbuffer_cov_ref, mixed, pad_word, temporal_cov_ref
from temporal_util import identity_xf, temporal_ref, translated, wall_camera
from test_device_bvh import _option_json
from test_temporal_host import ALPHA, H, W, WALL, frame, hostile, lerp

f32 = np.float32
FULL = pad_word(16, 16)
HIST = 5.0


def bits_equal(a, b):
    return all(np.array_equal(np.asarray(p).view(np.uint32), np.asarray(q).view(np.uint32)) for p, q in zip(a, b))


def pair(shift_x=0.0, shift_y=0.0, prev_cov=1, cur_cov=1):
    """Previous frame from the camera at the origin (history 5 everywhere), current frame from a camera shifted by that many pixel
    footprints; every pad word FULL."""
    prev = frame(wall_camera(), [WALL], seed=21, hist=HIST)
    cur = frame(wall_camera(shift_x / 3.0, shift_y / 3.0), [WALL], seed=22)
    prev["gbuffer"]["pad"], cur["gbuffer"]["pad"] = FULL, FULL
    prev["coverage"], cur["coverage"] = prev_cov, cur_cov
    return prev, cur


def kept_from(c, h, prev, cur, y, x, ys, xs):
    """Pixel (y, x) took its history from the one previous pixel (ys, xs) with weight 1: h = HIST + 1 and the colour is the lerp, exactly
    (S = 1, C / 1 = C)."""
    want = lerp(prev["color"][ys, xs, :3], cur["color"][y, x, :3], ALPHA)
    return h[y, x] == f32(HIST + 1) and np.array_equal(c[y, x, :3], want.astype(f32))


def restarted(c, v, h, cur, y, x):
    return h[y, x] == 1 and np.array_equal(c[y, x], cur["color"][y, x]) and v[y, x] == cur["variance"][y, x]


# ------------------------------------------------------------------------------------------------------------------ coverage off
@pytest.mark.parametrize("case", ["identity", "camera", "object", "hostile_cur", "hostile_prev", "no_prev"])
def test_coverage_zero_on_both_sides_is_temporal_ref_bit_for_bit(case):
    """With coverage 0 on both sides the pad words are ignored, whatever they hold: the checker's output is temporal_ref.cpp's bits."""
    cam = wall_camera()
    prev, cur = frame(cam, [WALL], seed=1, hist=4.0), frame(cam, [WALL], seed=2)
    if case == "camera":
        cur = frame(wall_camera(0.37, -0.21), [WALL], seed=2)
    if case == "object":
        m, inv = translated(identity_xf(2)[1:], identity_xf(2)[1:], (0.5, 0, 0))
        prev = frame(cam, [WALL, (-2.0, 1, 3, -0.5, 0.5)], (identity_xf(2), identity_xf(2)), seed=5, hist=7.0)
        cur = frame(cam, [WALL, (-2.0, 1, 3, 0.0, 1.0)], (np.concatenate([identity_xf(1), m]), np.concatenate([identity_xf(1), inv])), seed=6)
    if case == "hostile_cur":
        hostile(cur, False)
    if case == "hostile_prev":
        hostile(prev, True)
    rng = np.random.default_rng(3)
    for d in (prev, cur):
        d["gbuffer"]["pad"] = rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32)
    p = None if case == "no_prev" else prev
    want = temporal_ref(p, cur, 12)
    assert bits_equal(temporal_cov_ref(p, cur, 12), want)
    assert bits_equal(temporal_cov_ref(None if p is None else dict(p, coverage=0), dict(cur, coverage=0), 12), want)


def test_full_records_on_both_sides_change_nothing():
    """Coverage on both sides and no mixed record anywhere: rule 3' drops nothing and rule 2' never applies."""
    prev, cur = pair(0.4, -0.3)
    assert bits_equal(temporal_cov_ref(prev, cur, 12), temporal_ref(prev, cur, 12))


# ------------------------------------------------------------------------------------------------------------------ rule 2'
MIXED = pad_word(9, 16)
Y, X = 5, 7


@pytest.mark.parametrize("axis", ["x", "y"])
def test_snap_inside_and_outside(axis):
    """A mixed current pixel whose reprojection lies 0.1 pixel off a centre (inside HJR_TEMPORAL_SNAP = 0.125) takes that one pixel with
    weight 1; at 0.2 pixel (outside) it restarts; in x and in y separately, to either side.  Its full neighbours blend bilinearly as ever."""
    assert SNAP == f32(0.125) == hjr.TEMPORAL_SNAP
    for s, inside in ((0.1, True), (-0.1, True), (0.2, False), (-0.2, False), (1.1, True), (0.5, False)):
        prev, cur = pair(s if axis == "x" else 0.0, s if axis == "y" else 0.0)
        cur["gbuffer"]["pad"][Y, X] = MIXED
        prev["gbuffer"]["pad"][Y, X] = prev["gbuffer"]["pad"][Y + (axis == "y"), X + (axis == "x")] = MIXED  # (the pad test is not what this case is about)
        c, v, h = temporal_cov_ref(prev, cur, 12)
        ys, xs = (Y, X + int(round(s))) if axis == "x" else (Y + int(round(s)), X)
        if inside:
            assert kept_from(c, h, prev, cur, Y, X, ys, xs), "offset %.1f in %s: the one tap, weight 1" % (s, axis)
        else:
            assert restarted(c, v, h, cur, Y, X), "offset %.1f in %s: restart" % (s, axis)
        far = np.ones((H, W), bool)
        far[Y - 2:Y + 3, X - 2:X + 3] = False
        want = temporal_ref(prev, cur, 12)
        assert all(np.array_equal(g[far], w_[far]) for g, w_ in zip((c, v, h), want)), "pixels away from the mixed ones are untouched"


def test_snap_needs_both_axes():
    prev, cur = pair(0.1, 0.2)
    cur["gbuffer"]["pad"][Y, X] = prev["gbuffer"]["pad"][Y, X] = MIXED
    c, v, h = temporal_cov_ref(prev, cur, 12)
    assert restarted(c, v, h, cur, Y, X)
    c, v, h = temporal_cov_ref(prev, cur, 12, snap=0.25)
    assert kept_from(c, h, prev, cur, Y, X, Y, X), "(the checker's SNAP argument, for the re-tune of the rehearsal)"


def test_pad_mismatch_restarts_and_a_previous_side_without_coverage_does_not_compare():
    prev, cur = pair(0.05, 0.0)
    cur["gbuffer"]["pad"][Y, X] = MIXED
    prev["gbuffer"]["pad"][Y, X] = MIXED
    c, v, h = temporal_cov_ref(prev, cur, 12)
    assert kept_from(c, h, prev, cur, Y, X, Y, X), "equal pad words: kept"
    for other in (pad_word(10, 16), pad_word(9, 9), FULL, np.uint32(MIXED | 0x10000)):
        prev["gbuffer"]["pad"][Y, X] = other
        c, v, h = temporal_cov_ref(prev, cur, 12)
        assert restarted(c, v, h, cur, Y, X), "pad %#x against %#x: all 32 bits are compared" % (other, MIXED)
        c, v, h = temporal_cov_ref(dict(prev, coverage=0), cur, 12)
        assert kept_from(c, h, prev, cur, Y, X, Y, X), "the previous side carries no coverage: its pad is not looked at"


def test_the_one_tap_still_passes_rule_3():
    """The snapped tap is subject to the validity tests: another instance, a miss, or outside the image restart the pixel."""
    for poison in ("inst", "miss", "edge"):
        prev, cur = pair(-1.0 if poison == "edge" else 0.0, 0.0)
        y, x = (Y, 0) if poison == "edge" else (Y, X)
        cur["gbuffer"]["pad"][y, x] = MIXED
        prev["gbuffer"]["pad"][:] = MIXED
        if poison == "inst":
            prev["gbuffer"]["inst"][Y, X] = 1
        if poison == "miss":
            prev["gbuffer"]["prim"][Y, X] = 0xffffffff
        c, v, h = temporal_cov_ref(prev, cur, 12)
        assert restarted(c, v, h, cur, y, x), poison


# ------------------------------------------------------------------------------------------------------------------ rule 3'
def test_a_mixed_tap_is_dropped_from_a_full_pixel():
    """Offset 0.5 pixel in x: a full pixel blends previous pixels x and x + 1.  With x + 1 mixed only x is left and S = w0: the previous
    colour is prev[x] up to the rounding of (c * w) / w; without coverage on the previous side both taps stay."""
    prev, cur = pair(0.5, 0.0)
    prev["gbuffer"]["pad"][Y, X + 1] = MIXED
    c, v, h = temporal_cov_ref(prev, cur, 12)
    want = lerp(prev["color"][Y, X, :3], cur["color"][Y, X, :3], ALPHA)
    assert np.abs(c[Y, X, :3] - want).max() <= 1e-6 and abs(h[Y, X] - (HIST + 1)) <= 1e-5
    both = temporal_ref(prev, cur, 12)
    assert np.abs(both[0][Y, X, :3] - want).max() > 1e-3, "the plain rule mixes the two"
    assert bits_equal(temporal_cov_ref(dict(prev, coverage=0), cur, 12), both)
    changed = (c != both[0]).any(axis=-1)
    assert changed[Y, X] and changed[Y, X + 1] and changed.sum() == 2, "exactly the two pixels that tapped the mixed record differ"
    # all taps of a full pixel mixed: restart
    prev["gbuffer"]["pad"][:] = MIXED
    c, v, h = temporal_cov_ref(prev, cur, 12)
    assert (h == 1).all()


# ------------------------------------------------------------------------------------------------------------------ the mixed test itself
@pytest.mark.parametrize("word,name", [(5, "total = 0"), (pad_word(20, 16), "same > total"), (0xffffffff, "pad = 0xffffffff"), (pad_word(16, 16), "same == total"),
                                       (0, "pad = 0")])
def test_words_that_are_not_mixed(word, name):
    """total = 0, same > total (also same = total = 255 of an all-ones word) are not mixed: on either side such a record behaves as a full
    one, to the bit."""
    assert not mixed(np.array([(0,) * 5 + ((0, 0, 0), (0, 0, 0), word)], hjr.GBUFFER_DTYPE))[0]
    prev, cur = pair(0.5, 0.3)
    want = temporal_cov_ref(prev, cur, 12)
    rng = np.random.default_rng(4)
    for d in (prev, cur):
        d["gbuffer"]["pad"][rng.random((H, W)) < 0.5] = word
    assert bits_equal(temporal_cov_ref(prev, cur, 12), want), name
    assert (want[2] > 1).mean() > 0.7


def test_mixed_rule_examples():
    words = np.zeros(6, hjr.GBUFFER_DTYPE)
    words["pad"] = [pad_word(0, 4), pad_word(3, 4), pad_word(4, 4), pad_word(15, 16), pad_word(8, 9) | 0xabcd0000, 0x0000ff00]
    assert mixed(words).tolist() == [True, True, False, True, True, True]


# ------------------------------------------------------------------------------------------------------------------ the coverage pass of the checker
def test_checker_coverage_pass_on_two_triangles():
    """A quad at z = -4 (two triangles, two materials split along the diagonal, one instance) in front of the sky, 8 x 6, f = 2: pixels
    inside one triangle are full, pixels the diagonal or the quad's border crosses are mixed, sky pixels away from the quad are full misses,
    and side 0 is the plain record with pad = 0."""
    rows = np.zeros((2, 12), f32)
    rows[0, :9] = [-1, -1, -4, 1, -1, -4, 1, 1, -4]
    rows[1, :9] = [-1, -1, -4, 1, 1, -4, -1, 1, -4]
    rows[:, 9] = np.array([0, 1], np.uint32).view(f32)
    inst = np.zeros(2, np.uint32)
    cam = wall_camera()
    for side in (2, 3, 4):
        g = gbuffer_cov_ref(rows, inst, np.array([0, 1], np.uint32), 8, 6, cam, side)
        g1 = gbuffer_cov_ref(rows, inst, np.array([0, 0], np.uint32), 8, 6, cam, side)
        g0 = gbuffer_cov_ref(rows, inst, np.array([0, 1], np.uint32), 8, 6, cam, 0)
        assert ((g["pad"] >> 8) == side * side).all() and (g0["pad"] == 0).all()
        for name in ("prim", "inst", "t", "b1", "b2", "pos", "ng"):
            assert np.array_equal(g[name].view(np.uint32), g0[name].view(np.uint32)), name
        miss = g["prim"] == 0xffffffff
        assert miss.any() and not miss.all()
        assert not g0[miss].tobytes().replace(b"\xff\xff\xff\xff", b"").strip(b"\0")
        # the quad spans u, v in [-0.5, 0.5]: x in [2.5, 5.5) and y in [1.5, 4.5) in pixel units: rows 1 and 4 and columns 2 and 5 are cut by its border
        m = mixed(g)
        assert m[1, 2:6].all() and m[4, 2:6].all() and m[1:5, 2].all() and m[1:5, 5].all()
        assert not m[:, :2].any() and not m[:, 6:].any() and not m[0].any() and not m[5].any()
        # one material: the diagonal no longer separates anything
        assert not mixed(g1)[2:4, 3:5].any() and m[2:4, 3:5].any()
        assert (g["pad"][0] == pad_word(side * side, side * side)).all(), "a sky pixel away from the quad: every sub-ray misses too"


# ------------------------------------------------------------------------------------------------------------------ option table and file key
def test_option_table_entry(tmp_path):
    """host/options.hpp: the key exists, its range is 0..4 and 1 is refused inside it, as 3 is for "bvh_width"."""
    src = tmp_path / "opt.cpp"
    src.write_text("""
#include <cstdio>
#include "options.hpp"
int main() {
    const int i = hjr::opt_find("denoise_temporal_coverage");
    if (i < 0) return 1;
    printf("%d %d", hjr::opt_table()[i].lo, hjr::opt_table()[i].hi);
    for (int v = -2; v <= 6; v++) printf(" %d", (v == -1 || (v >= hjr::opt_table()[i].lo && v <= hjr::opt_table()[i].hi && !hjr::opt_hole(i, v))) ? 1 : 0);
    printf(" %d\\n", hjr::opt_hole(hjr::opt_find("bvh_width"), 3) ? 1 : 0);
    return 0;
}
""")
    exe = str(tmp_path / "opt")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "henjou-renderer_amd", "host"), str(src), "-o", exe])
    out = list(map(int, subprocess.check_output([exe]).decode().split()))
    assert out[:2] == [0, 4]
    assert out[2:11] == [0, 1, 1, 0, 1, 1, 1, 0, 0], "accepted: -1 (default), 0, 2, 3, 4; refused: -2, 1, 5, 6"
    assert out[11] == 1


def test_render_option_key(tmp_path):
    """"Henjou_HIP": {"denoise_temporal_coverage": N} is stored in bits 12..14 of hjr_render_option.device_bvh_opt next to the other keys
    of the field and read back from there; 0, 2, 3, 4 are accepted, everything else is a parse error; the struct does not grow."""
    load = lambda extra: hjr.load_render_option(_option_json(tmp_path, extra))  # noqa: E731
    for extra in (None, {}, {"denoise_temporal_coverage": 0}, {"denoise_temporal": True}):
        assert load(extra).device_bvh_opt == 0
    for n in (2, 3, 4):
        o = load({"denoise_temporal_coverage": n, "denoise_temporal": True})
        assert o.device_bvh_opt == n << 12 and (o.device_bvh_opt >> 12) & 7 == n and o.denoise_variance == 2
        assert load({"denoise_temporal_coverage": n}).device_bvh_opt == n << 12, "accepted without denoise_temporal (no effect)"
    o = load({"denoise_temporal_coverage": 4, "upscale_guided": True, "denoise_variance_spatial": True, "firefly_clamp": 64, "device_bvh": True, "device_bvh_opt": 3,
              "device_bvh_instances": True, "device_bvh_graft": True})
    assert o.device_bvh_opt == 3 | 0x100 | 0x200 | 0x400 | 0x800 | (4 << 12) | (64 << 16)
    for bad in (1, 5, 8, -1, 2.5, True, "4", None, [4]):
        with pytest.raises(hjr.HjrError, match="denoise_temporal_coverage"):
            load({"denoise_temporal_coverage": bad})
    assert hjr.RenderOption.denoise_variance.offset + 4 == C.sizeof(hjr.RenderOption), "nothing was appended"


def test_struct_field_and_constant(tmp_path):
    """hjr_temporal_frame grew at its end by `coverage` only (every earlier offset is what tests/test_temporal_host.py pins), the ctypes
    mirror agrees, and HJR_TEMPORAL_SNAP is 0.125f."""
    src = tmp_path / "off.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "henjou_hip.h"
int main(void) {
    printf("%zu %zu %zu %.9g\\n", offsetof(hjr_temporal_frame, history), offsetof(hjr_temporal_frame, coverage), sizeof(hjr_temporal_frame), (double)HJR_TEMPORAL_SNAP);
    return 0;
}
""")
    exe = str(tmp_path / "off")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    hist, cov, size, snap = subprocess.check_output([exe]).decode().split()
    F = hjr.TemporalFrame
    assert [int(hist), int(cov), int(size)] == [F.history.offset, F.coverage.offset, C.sizeof(F)]
    assert int(cov) == int(hist) + 8 and F._fields_[-1][0] == "coverage"
    assert f32(float(snap)) == SNAP
    L = hjr.lib()
    assert L.hjr_render_gbuffer_cov(None, None, 1, None) == -1 and L.hjr_render_gbuffer_cov_device(None, None, 5, None, None) == -1
    assert b"side" in L.hjr_last_error()
    assert L.hjr_render_gbuffer_cov(None, None, 4, None) == -1
