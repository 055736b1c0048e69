"""Host-only parts of the temporal luminance moments (hjr_temporal_accumulate_moments, option "denoise_temporal_moments";
csrc/hjr_temporal.hip.h section TEMPORAL MOMENTS): the semantics of the native checker the GPU kernel is compared with
(tests/native/temporal_moments_ref.cpp) on the synthetic 16 x 12 plane frames of tests/test_temporal_host.py, the struct field and the
constant, the "denoise_temporal_moments" key of the render option, and the CPU rehearsal of the quality comparison.  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from scene_util import ROOT, Cornell, hjr
from temporal_cov_util import pad_word, temporal_cov_ref
from temporal_moments_util import K_LIMIT, MOMENTS_MIN, UNKNOWN, temporal_moments_ref
from temporal_util import assert_same, identity_xf, luminance, next_prev, same_bits, temporal_ref, translated, wall_camera
from test_device_bvh import _option_json
from test_temporal_host import H, W, WALL, frame

f32 = np.float32


def with_moments(d, seed):
    d["moments"] = np.random.default_rng(seed).uniform(0.1, 0.9, (H, W, 2)).astype(f32)
    return d


def moving_pair(seed=5, hist=7.0):
    """tests/test_temporal_host.py's moving strip: taps rejected, pixels that restart, pixels that follow the object."""
    cam = wall_camera()
    m, inv = translated(identity_xf(2)[1:], identity_xf(2)[1:], (0.5, 0, 0))
    xf_cur = (np.concatenate([identity_xf(1), m]), np.concatenate([identity_xf(1), inv]))
    prev = frame(cam, [WALL, (-2.0, 1, 3, -0.5, 0.5)], (identity_xf(2), identity_xf(2)), seed=seed, hist=hist)
    cur = frame(cam, [WALL, (-2.0, 1, 3, 0.0, 1.0)], xf_cur, seed=seed + 1)
    return prev, cur


def test_moments_disabled_is_the_plain_checker():
    """MOMENTS 0: the bits of tests/native/temporal_ref.cpp on the plane frames (identity, a moved camera, the moving strip, no previous
    frame, hostile variances), and those of temporal_cov_ref.cpp with coverage flags and mixed pad words."""
    cam = wall_camera()
    pairs = [(frame(cam, [WALL], seed=1, hist=2.0), frame(cam, [WALL], seed=2)),
             (frame(wall_camera(0.0), [WALL], seed=3, hist=5.0), frame(wall_camera(0.9), [WALL], seed=4)),
             moving_pair(), (None, frame(cam, [WALL], seed=2))]
    bad_p, bad_c = frame(cam, [WALL], seed=9, hist=4.0), frame(cam, [WALL], seed=10)
    bad_p["variance"][2, 3] = UNKNOWN; bad_p["variance"][5, 9] = np.nan; bad_p["variance"][4, 4] = -1.0; bad_c["variance"][7, 12] = np.inf
    pairs.append((bad_p, bad_c))
    for prev, cur in pairs:
        assert_same(temporal_moments_ref(prev, cur, 12, moments=False), temporal_ref(prev, cur, 12), "plain")
    prev, cur = moving_pair()
    rng = np.random.default_rng(3)
    for d in (prev, cur):
        d["coverage"] = 2
        d["gbuffer"]["pad"] = np.where(rng.random((H, W)) < 0.3, pad_word(2, 4), pad_word(4, 4))
    for pc, cc in ((2, 2), (0, 2), (2, 0)):
        p, c = dict(prev, coverage=pc), dict(cur, coverage=cc)
        assert_same(temporal_moments_ref(p, c, 12, moments=False), temporal_cov_ref(p, c, 12), "coverage %d %d" % (pc, cc))
        with_m = temporal_moments_ref(with_moments(dict(p), 1), c, 12)
        assert_same(with_m[:1] + with_m[2:3], temporal_cov_ref(p, c, 12)[:1] + temporal_cov_ref(p, c, 12)[2:3], "colour and history with moments")


def test_restart_gives_l_and_l_squared():
    """No previous frame, misses and disoccluded pixels: m1 = l, m2 = l * l of the current colour; colour, variance and h as without."""
    cam = wall_camera()
    cur = frame(cam, [WALL], seed=2)
    c, v, h, m = temporal_moments_ref(None, cur, 12)
    l = luminance(cur["color"])
    assert same_bits(m[..., 0], l) and same_bits(m[..., 1], l * l)
    assert same_bits(c, cur["color"]) and same_bits(v, cur["variance"]) and (h == 1).all()
    prev, cur = moving_pair()
    c, v, h, m = temporal_moments_ref(with_moments(prev, 1), cur, 12)
    restart = h == 1
    assert restart[:, 6:8].all() and not restart[:, 8:14].any()
    l = luminance(cur["color"])
    assert same_bits(m[restart][:, 0], l[restart]) and same_bits(m[restart][:, 1], (l * l)[restart])
    assert not np.array_equal(m[~restart][:, 0], l[~restart])
    plain = temporal_ref(prev, cur, 12)
    assert same_bits(c, plain[0]) and same_bits(h, plain[2])
    assert same_bits(v[restart], plain[1][restart])


def test_constant_luminance_switches_at_four():
    """A chain of frames of one constant colour on the wall: below h = 4 a pixel carries the propagated variance (the plain checker's), from
    h = 4 on its variance is exactly 0, and the moments stay (l, l * l).  l = 0.5 and l * l = 0.25 are powers of two, so the weighted sums
    are exact multiples of the weight sum whatever the weights are.  The reprojection lands within 2e-6 of a pixel centre, not on it, so a
    history of 3 can come back as 3 - 2^-22 and the pixel then switches one frame later: frame 4 is checked per pixel."""
    cam = wall_camera()
    prev_m = prev_p = None
    for f in range(1, 8):
        cur = frame(cam, [WALL], seed=20 + f)
        cur["color"][..., :3] = f32(0.25), f32(0.125), f32(0.125)
        out = temporal_moments_ref(prev_m, cur, 12)
        plain = temporal_ref(prev_p, cur, 12)
        assert np.abs(out[2] - f).max() <= 1e-4
        assert same_bits(out[0], plain[0]) and same_bits(out[2], plain[2])
        switched = out[2] >= MOMENTS_MIN
        assert not switched.any() if f < 4 else switched.all() if f > 4 else switched.mean() > 0.25, "frame %d" % f
        assert (out[1][switched] == 0).all(), "frame %d: var = 0 from h = 4 on" % f
        assert same_bits(out[1][~switched], plain[1][~switched]), "frame %d: the propagated variance below" % f
        assert (out[3][..., 0] == f32(0.5)).all() and (out[3][..., 1] == f32(0.25)).all()
        prev_m, prev_p = next_prev(cur, out), dict(cur, color=plain[0], variance=plain[1], history=plain[2])


def test_variance_formula_at_and_above_the_switch():
    """One step from a uniform history: h_prev = 4 (k = 1 / 5; a power of two comes back exactly) and h_prev = 40 (k = alpha / (2 - alpha))
    against the formula in float64."""
    cam = wall_camera()
    for h_prev, k in ((4.0, 0.2), (40.0, float(K_LIMIT))):
        prev, cur = with_moments(frame(cam, [WALL], seed=31, hist=h_prev), 7), frame(cam, [WALL], seed=32)
        prev["moments"][..., 1] += 1  # m2 well above m1 * m1
        c, v, h, m = temporal_moments_ref(prev, cur, 12)
        al = max(1.0 / (h_prev + 1), 0.2)
        l = luminance(cur["color"]).astype(np.float64)
        # (the reprojection lands within 2e-6 of the pixel's own centre: the second taps weigh that little)
        m1 = prev["moments"][..., 0] + (l - prev["moments"][..., 0]) * al
        m2 = prev["moments"][..., 1] + (l * l - prev["moments"][..., 1]) * al
        assert np.abs(m[..., 0] - m1).max() <= 1e-5 and np.abs(m[..., 1] - m2).max() <= 1e-5
        want = np.maximum(m2 - m1 * m1, 0) * k / (1 - k)
        assert np.abs(v - want).max() <= 1e-5 * want.max() + 1e-6
        assert (v > 0).all()
    # below the switch the moments are kept and the variance is the plain one
    prev, cur = with_moments(frame(cam, [WALL], seed=31, hist=2.0), 7), frame(cam, [WALL], seed=32)
    assert same_bits(temporal_moments_ref(prev, cur, 12)[1], temporal_ref(prev, cur, 12)[1])
    # an unknown propagated variance does not matter at the switch, and stays below it
    for hist, known in ((4.0, True), (2.0, False)):
        prev = with_moments(frame(cam, [WALL], seed=31, hist=hist), 7)
        prev["variance"][:] = UNKNOWN
        v = temporal_moments_ref(prev, cur, 12)[1]
        assert ((v < UNKNOWN).all() and np.isfinite(v).all()) if known else (v == UNKNOWN).all()


def hostile_moments(m):
    """Poisons moments in place: NaN, +-Inf, 1e38 (m1 * m1 overflows), 3e38 in m2, a negative m2.  Returns the mask."""
    vals = [(np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (-np.inf, 0.5), (0.5, np.inf), (0.5, -np.inf), (1e38, 0.5), (-1e38, 1e38), (0.5, 3e38), (0.5, -4.0), (np.nan, np.nan)]
    bad = np.zeros(m.shape[:2], bool)
    for i, (a, b) in enumerate(vals):
        y, x = 1 + 2 * (i // 6), 1 + 2 * (i % 6)
        m[y, x] = (a, b)
        bad[y, x] = True
    return bad


def test_hostile_moments_end_unknown_or_finite():
    cam = wall_camera()
    for hist in (2.0, 4.0, 30.0):
        prev, cur = with_moments(frame(cam, [WALL], seed=41, hist=hist), 9), frame(cam, [WALL], seed=42)
        bad = hostile_moments(prev["moments"])
        c, v, h, m = temporal_moments_ref(prev, cur, 12)
        assert not np.isnan(v).any() and ((v == UNKNOWN) | (np.isfinite(v) & (v >= 0) & (v < UNKNOWN))).all()
        plain = temporal_ref(prev, cur, 12)
        assert same_bits(c, plain[0]) and same_bits(h, plain[2]), "colour and history never see the moments"
        if hist >= 4.0:
            assert (v[bad] == UNKNOWN).sum() >= 9, "NaN, Inf and overflowing squares are unknown"
            assert v[3, 7] == 0, "a negative m2 gives a negative difference: clamped to 0"
        else:
            assert same_bits(v, plain[1])


def test_struct_field_and_constant(tmp_path):
    """hjr_temporal_frame is the struct it was (128 bytes, `coverage` at 120 its last field: the previous moments are an argument of the new
    entry points, not a field), the ctypes mirror agrees, the new entry points are declared with eight and nine arguments, and
    HJR_TEMPORAL_MOMENTS_MIN is 4."""
    src = tmp_path / "off.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "henjou_hip.h"
int (*host_form)(hjr_ctx*, const hjr_temporal_frame*, const hjr_temporal_frame*, float*, float*, float*, const float*, float*) = hjr_temporal_accumulate_moments;
int (*device_form)(hjr_ctx*, const hjr_temporal_frame*, const hjr_temporal_frame*, void*, void*, void*, const void*, void*, void*) = hjr_temporal_accumulate_moments_device;
int main(void) {
    printf("%zu %zu %.9g\\n", offsetof(hjr_temporal_frame, coverage), sizeof(hjr_temporal_frame), (double)HJR_TEMPORAL_MOMENTS_MIN);
    return host_form == 0 || device_form == 0;
}
""")
    exe = str(tmp_path / "off")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + hjr.PKG_DIR, "-lhenjou_hip",
                           "-Wl,-rpath," + hjr.PKG_DIR, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().split()
    F = hjr.TemporalFrame
    assert list(map(int, out[:2])) == [120, 128] == [F.coverage.offset, C.sizeof(F)] and F._fields_[-1][0] == "coverage"
    assert f32(float(out[2])) == hjr.TEMPORAL_MOMENTS_MIN == MOMENTS_MIN == 4
    L = hjr.lib()
    assert L.hjr_temporal_accumulate_moments(None, None, None, None, None, None, None, None) == -1
    assert L.hjr_temporal_accumulate_moments_device(None, None, None, None, None, None, None, None, None) == -1


NATIVE_KEY_TEST = r"""
#include <cstdio>
#include <string>
#include "render_job.hpp"
int main()
{
    using namespace hjr;
    int seen = 0;
    for (const KeyRow& r : key_rows()) if (std::string(r.key) == "denoise_temporal_moments") seen++;
    const KeyRow& r = key_row("denoise_temporal_moments");
    if (seen != 1 || std::string(r.key) != "denoise_temporal_moments" || r.field != &hjr_render_option::device_bvh_opt || r.enc != ENC_BITS || r.shift != 15 || r.width != 1 ||
        r.read != READ_BOOL || r.needs || r.who != WHO_FILTER || &r != &key_rows().back()) { printf("row\n"); return 1; }
    for (const KeyRow& q : key_rows())
        if (&q != &r && q.field == r.field && q.enc == ENC_BITS && q.shift <= 15 && q.shift + q.width > 15) { printf("bit 15 is taken by %s\n", q.key); return 1; }
    for (const KeyRow& q : key_rows()) if (&q != &r && q.parse >= r.parse) { printf("parse turn\n"); return 1; }
    hjr_render_option o;
    HJR_INIT(o);
    key_put(o, key_row("denoise_temporal_coverage"), 4);
    key_put(o, key_row("firefly_clamp"), 64);
    key_put(o, r, 1);
    if (o.device_bvh_opt != ((4 << 12) | (64 << 16) | (1 << 15)) || key_get(o, r) != 1 || key_get(o, key_row("denoise_temporal_coverage")) != 4 ||
        key_get(o, key_row("firefly_clamp")) != 64 || key_get(o, key_row("device_bvh_opt")) != 0) { printf("pack\n"); return 1; }
    for (int mode : { (int)HJR_MODE_DEFAULT, (int)HJR_MODE_DENOISE, (int)HJR_MODE_DENOISE_UPSCALE2X })
        for (int temporal = 0; temporal < 2; temporal++) {
            hjr_render_option p;
            HJR_INIT(p);
            p.render_mode = mode; p.image_width = 16; p.image_height = 8;
            key_put(p, r, 1);
            if (temporal) key_put(p, key_row("denoise_temporal"), 1);
            Job job;
            std::string text;
            if (!job_check(p, job, text)) { printf("job_check refuses: %s\n", text.c_str()); return 1; }
            std::string mine, other;
            for_each_option(p, single_process(), [&](const char* k, int v) { mine += std::string(k) + "=" + std::to_string(v) + " "; return 0; });
            for_each_option(p, rank_of_world(1), [&](const char* k, int v) { other += std::string(k) + "=" + std::to_string(v) + " "; return 0; });
            const std::string want = std::string(temporal && mode != HJR_MODE_DEFAULT ? "denoise_variance=1 denoise_temporal=1 " : "") + "denoise_temporal_moments=1 ";
            if (mine != want || !other.empty()) { printf("options: [%s] [%s], want [%s]\n", mine.c_str(), other.c_str(), want.c_str()); return 1; }
        }
    printf("key ok\n");
    return 0;
}
"""


def test_file_key_row_packs_and_job_check_accepts_it(tmp_path):
    """The row of key_table_since(): strict bool, bit 15 of device_bvh_opt (free of every other row), WHO_FILTER, the last parse turn; it
    packs next to its neighbours and round-trips through key_rows(); job_check accepts it with and without "denoise_temporal" in all three
    modes; the single process and rank 0 set the option, the other ranks do not."""
    src = tmp_path / "key.cpp"
    src.write_text(NATIVE_KEY_TEST)
    exe = str(tmp_path / "key")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(hjr.PKG_DIR, "host"), str(src), "-o", exe,
                           "-L" + hjr.PKG_DIR, "-lhenjou_hip", "-Wl,-rpath," + hjr.PKG_DIR, "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "key ok" in p.stdout, p.stdout + p.stderr


def test_render_option_reads_the_key(tmp_path):
    load = lambda s: hjr.load_render_option(_option_json(tmp_path, s))
    assert load({"denoise_temporal_moments": True}).device_bvh_opt == 1 << 15
    assert load({"denoise_temporal_moments": 1, "denoise_temporal": True, "denoise_variance_spatial": True}).device_bvh_opt == (1 << 15) | (1 << 10)
    assert load({"denoise_temporal_moments": 1, "denoise_temporal": True}).denoise_variance == 2
    assert load({"denoise_temporal_moments": True, "denoise_temporal_coverage": 4, "firefly_clamp": 64}).device_bvh_opt == (1 << 15) | (4 << 12) | (64 << 16)
    for off in (False, 0):
        assert load({"denoise_temporal_moments": off}).device_bvh_opt == 0
    assert load({}).device_bvh_opt == 0
    for bad in (2, -1, "1", 0.5, None):
        with pytest.raises(hjr.HjrError, match="denoise_temporal_moments"):
            load({"denoise_temporal_moments": bad})


def test_rehearsal_prints_its_table():
    """tools/temporal_moments_rehearsal.py at 48 x 32, 4 spp, references of 256 spp: the stages run end to end on the oracle's frames and
    the table has its four columns for both sequences.  Frames 1..3 do not depend on the moments; from frame 4 on the static chain does,
    and with the moments the spatial estimate no longer matters there (every pixel's history is long enough).  The quality conditions are
    those of 96 x 64 with 4096 spp references (tests/test_gpu_temporal_moments.py): printed here, not asserted."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import temporal_moments_rehearsal as tmr
    from temporal_moments_util import format_tables, quality_conditions
    tables = tmr.rehearse(Cornell(), 48, 32, 256, spps=(4,))
    print(format_tables(tables))
    for text, holds in quality_conditions(tables):
        print("%s: %s (48 x 32: not asserted)" % (text, "holds" if holds else "fails"))
    assert set(tables) == {("static", 4), ("moving", 4)}
    for t in tables.values():
        assert all(len(t[k]) == 8 and np.isfinite(t[k]).all() for k in ("spatial", "spatial+moments", "unknown", "moments"))
        assert t["spatial"][:3] == t["spatial+moments"][:3] and t["unknown"][:3] == t["moments"][:3]
    s = tables[("static", 4)]
    assert s["spatial"][3:] != s["spatial+moments"][3:] and s["moments"][3:] == s["spatial+moments"][3:]
