"""Host-only parts of the windowed change test of the temporal accumulation (hjr_temporal_accumulate_response, option
"denoise_temporal_response"; csrc/hjr_temporal.hip.h section RESPONSE): the native checker the GPU kernel is compared
with (tests/native/temporal_response_ref.cpp) against the numpy restatement of the section and against the older checkers, the constants and
entry points of the header, the option row, the "denoise_temporal_response" key of the render option and its bit, job_check's texts, and
the CPU rehearsal.  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from scene_util import ROOT, Cornell, hjr
from temporal_cov_util import pad_word
from temporal_moments_util import temporal_moments_ref
from temporal_response_util import (P_SPLIT, P_TRIS, PH, PW, RESP_EPS, RESP_NMIN, RESP_R, RESP_T0, RESP_T1, blend_numpy, check_planes_lambda, light_instance,
                                    planes_case, response_numpy, sequence_transforms, temporal_response_ref)
from temporal_util import MISS, assert_same, same_bits, temporal_ref
from test_device_bvh import _option_json

f32 = np.float32


def carried_of(prev, cur, n_tris):
    """The carried mask from the plain checker: with every previous history >= 1 a carried pixel ends with h > 1."""
    return temporal_ref(prev, cur, n_tris)[2] > 1


def test_checker_equals_numpy_on_the_planes_case():
    """tests/native/temporal_response_ref.cpp against response_numpy / blend_numpy (sections RESPONSE and step 4 in numpy float32) on the
    synthetic planes: lambda, colour, variance and history bit for bit, and lambda is what the construction says."""
    prev, cur, c_prev = planes_case()
    carried = carried_of(prev, cur, P_TRIS)
    hit = cur["gbuffer"]["prim"] != MISS
    assert np.array_equal(carried, hit) and (~hit).sum() == 16
    c, v, h, lam = temporal_response_ref(prev, cur, P_TRIS)
    want = response_numpy(cur["color"], c_prev, carried, cur["gbuffer"], P_TRIS)
    assert same_bits(lam, want)
    check_planes_lambda(lam, "checker")
    bc, bv, bh = blend_numpy(cur["color"], cur["variance"], c_prev, f32(2.0 ** -6), f32(8.0), carried, lam)
    assert same_bits(c, bc) and same_bits(v, bv) and same_bits(h, bh)
    assert (h[lam == 1] == 1).all() and (h[(lam == 0) & carried] == 9).all(), "lambda = 1 starts over, lambda = 0 leaves h alone"
    part = (lam > 0) & (lam < 1)
    assert part.any() and ((h[part] > 1) & (h[part] < 5)).all(), "h = min(h, 1 / al')"
    # another radius is another window: the one re-tune the rehearsal may ask for
    lam3 = temporal_response_ref(prev, cur, P_TRIS, radius=3)[3]
    assert same_bits(lam3, response_numpy(cur["color"], c_prev, carried, cur["gbuffer"], P_TRIS, radius=3)) and not same_bits(lam3, lam)


def test_lambda_zero_leaves_the_plain_bits():
    """The same frame accumulated onto itself as history: lambda = 0 everywhere and all outputs are the bits of the checkers without the
    change test, in all four forms (coverage flags with mixed pad words, moments); RESPONSE 0 is those checkers too."""
    prev, cur, _ = planes_case()
    same = dict(prev, color=cur["color"])
    rng = np.random.default_rng(5)
    for coverage in (0, 2):
        p, c = dict(same), dict(cur)
        if coverage:
            pads = np.where(rng.random((PH, PW)) < 0.3, pad_word(2, 4), pad_word(4, 4)).astype(np.uint32)
            for d in (p, c):
                d["coverage"] = coverage
                d["gbuffer"] = d["gbuffer"].copy()
                d["gbuffer"]["pad"] = pads
        for moments in (False, True):
            if moments:
                p["moments"] = rng.uniform(0.1, 0.9, (PH, PW, 2)).astype(f32)
            plain = temporal_moments_ref(p, c, P_TRIS, moments=moments)
            out = temporal_response_ref(p, c, P_TRIS, moments=moments)
            assert (out[-1] == 0).all()
            assert_same(out[:-1] + (out[-1],), plain + (np.zeros((PH, PW), f32),), "coverage %d moments %d" % (coverage, moments), moments)
            off = temporal_response_ref(p, c, P_TRIS, moments=moments, response=False)
            assert len(off) == len(plain) and all(same_bits(a, b) for a, b in zip(off, plain))
            # ... and the raised frame does differ from the plain rule
            raised = temporal_response_ref(dict(p, color=prev["color"]), c, P_TRIS, moments=moments)
            assert (raised[-1] > 0).any() and not same_bits(raised[0], temporal_moments_ref(dict(p, color=prev["color"]), c, P_TRIS, moments=moments)[0])


def test_restart_pixels_and_no_previous_frame():
    prev, cur, _ = planes_case()
    c, v, h, lam = temporal_response_ref(None, cur, P_TRIS)
    assert same_bits(c, cur["color"]) and same_bits(v, cur["variance"]) and (h == 1).all() and (lam == 0).all()
    c, v, h, lam = temporal_response_ref(prev, cur, P_TRIS)
    miss = cur["gbuffer"]["prim"] == MISS
    assert same_bits(c[miss], cur["color"][miss]) and (h[miss] == 1).all() and (lam[miss] == 0).all()


def test_hostile_luminances_give_a_lambda_in_range():
    """NaN / Inf / huge colours on both sides, a NaN history, the unknown variance: lambda is in [0, 1], a NaN t gives 0, and the numpy
    restatement agrees bit for bit (c_prev of the poisoned pixels is whatever the taps give: taken from the constant history elsewhere)."""
    prev, cur, c_prev = planes_case()
    cur["color"][3, 3, 0] = np.nan; cur["color"][5, 6, 1] = np.inf; cur["color"][9, 4, 2] = -np.inf; cur["color"][12, 8, 0] = 3e38; cur["color"][14, 25, 0] = -3e38
    prev["variance"][2, 2] = 1e30; cur["variance"][7, 7] = np.nan
    c, v, h, lam = temporal_response_ref(prev, cur, P_TRIS)
    assert np.isfinite(lam).all() and (lam >= 0).all() and (lam <= 1).all()
    assert same_bits(lam, response_numpy(cur["color"], c_prev, carried_of(prev, cur, P_TRIS), cur["gbuffer"], P_TRIS))
    assert (lam[1:6, 1:6] == 0).all(), "a NaN in the window: t is NaN, lambda 0"
    assert v[2, 2] == f32(1e30) and v[7, 7] == f32(1e30)
    # out-of-range ids are no members and restart
    cur["gbuffer"]["inst"][10, 10] = 0xffffffff; cur["gbuffer"]["prim"][10, 12] = 1 << 30
    c, v, h, lam = temporal_response_ref(prev, cur, P_TRIS)
    assert lam[10, 10] == 0 and lam[10, 12] == 0 and h[10, 10] == 1 and h[10, 12] == 1


def test_constants_entry_points_and_struct(tmp_path):
    """HJR_TEMPORAL_RESP_* are the issue's, hjr_temporal_frame keeps its 128 bytes, the new entry points are declared with nine and ten
    arguments and refuse NULL, and the ctypes mirror of the constants agrees."""
    src = tmp_path / "resp.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "henjou_hip.h"
int (*host_form)(hjr_ctx*, const hjr_temporal_frame*, const hjr_temporal_frame*, float*, float*, float*, const float*, float*, float*) = hjr_temporal_accumulate_response;
int (*device_form)(hjr_ctx*, const hjr_temporal_frame*, const hjr_temporal_frame*, void*, void*, void*, const void*, void*, void*, void*) = hjr_temporal_accumulate_response_device;
int main(void) {
    printf("%d %.9g %.9g %d %.9g %zu\\n", HJR_TEMPORAL_RESP_R, (double)HJR_TEMPORAL_RESP_T0, (double)HJR_TEMPORAL_RESP_T1, HJR_TEMPORAL_RESP_NMIN,
           (double)HJR_TEMPORAL_RESP_EPS, sizeof(hjr_temporal_frame));
    return host_form == 0 || device_form == 0;
}
""")
    exe = str(tmp_path / "resp")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + hjr.PKG_DIR, "-lhenjou_hip",
                           "-Wl,-rpath," + hjr.PKG_DIR, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().split()
    assert int(out[0]) == 2 == RESP_R == hjr.TEMPORAL_RESP["R"] and int(out[3]) == 5 == RESP_NMIN == hjr.TEMPORAL_RESP["NMIN"]
    assert f32(float(out[1])) == f32(3) == RESP_T0 == hjr.TEMPORAL_RESP["T0"] and f32(float(out[2])) == f32(6) == RESP_T1 == hjr.TEMPORAL_RESP["T1"]
    assert f32(float(out[4])) == f32(1e-3) == RESP_EPS == hjr.TEMPORAL_RESP["EPS"]
    assert int(out[5]) == 128 == C.sizeof(hjr.TemporalFrame)
    L = hjr.lib()
    assert L.hjr_temporal_accumulate_response(None, None, None, None, None, None, None, None, None) == -1
    assert L.hjr_temporal_accumulate_response_device(None, None, None, None, None, None, None, None, None, None) == -1


NATIVE_KEY_TEST = r"""
#include <cstdio>
#include <string>
#include "options.hpp"
#include "render_job.hpp"
int main()
{
    using namespace hjr;
    const int oi = opt_find("denoise_temporal_response");
    if (oi != OPT_DENOISE_TEMPORAL_RESPONSE || opt_table()[oi].lo != 0 || opt_table()[oi].hi != 1) { printf("option row\n"); return 1; }
    int seen = 0, in_since = 0;
    for (const KeyRow& r : key_rows()) if (std::string(r.key) == "denoise_temporal_response") seen++;
    for (const KeyRow& r : key_table_since()) if (std::string(r.key) == "denoise_temporal_response") in_since++;
    for (const KeyRow& r : key_table()) if (std::string(r.key) == "denoise_temporal_response") { printf("key_table() grew\n"); return 1; }
    const KeyRow& r = key_row("denoise_temporal_response");
    if (seen != 1 || in_since != 1 || key_table().size() != 13 || std::string(r.key) != "denoise_temporal_response" || r.field != &hjr_render_option::device_bvh_opt ||
        r.enc != ENC_BITS || r.shift != 24 || r.width != 1 || r.read != READ_BOOL || r.needs || r.who != WHO_FILTER) { printf("row\n"); return 1; }
    for (const KeyRow& q : key_rows()) {
        if (&q != &r && q.field == r.field && q.enc == ENC_BITS && q.shift <= 24 && q.shift + q.width > 24) { printf("bit 24 is taken by %s\n", q.key); return 1; }
        if (&q != &r && q.parse == r.parse) { printf("parse turn shared with %s\n", q.key); return 1; }
    }
    hjr_render_option o;
    HJR_INIT(o);
    key_put(o, key_row("firefly_clamp"), 64);
    key_put(o, key_row("firefly_clamp_passes"), 1);
    key_put(o, key_row("denoise_temporal_moments"), 1);
    key_put(o, r, 1);
    if (o.device_bvh_opt != ((64 << 16) | (1 << 23) | (1 << 15) | (1 << 24)) || key_get(o, r) != 1 || key_get(o, key_row("firefly_clamp")) != 64 ||
        key_get(o, key_row("firefly_clamp_passes")) != 1 || key_get(o, key_row("denoise_temporal_moments")) != 1) { printf("pack\n"); return 1; }
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
            const std::string want = std::string(temporal && mode != HJR_MODE_DEFAULT ? "denoise_variance=1 denoise_temporal=1 " : "") + "denoise_temporal_response=1 ";
            if (mine != want || !other.empty()) { printf("options: [%s] [%s], want [%s]\n", mine.c_str(), other.c_str(), want.c_str()); return 1; }
            // the refusal together with "noise_threshold" stays, with its text
            p.noise_threshold = 0.01f;
            const bool ok = job_check(p, job, text);
            const bool refused = temporal && mode != HJR_MODE_DEFAULT;
            if (ok == refused || (refused && text.find("\"denoise_temporal\" cannot be combined with \"noise_threshold\"") == std::string::npos)) { printf("noise_threshold: %s\n", text.c_str()); return 1; }
        }
    printf("key ok\n");
    return 0;
}
"""


def test_option_row_key_row_and_job_check(tmp_path):
    """The option row (0..1), the row of key_table_since(): strict bool, bit 24 of device_bvh_opt (free of every other row), WHO_FILTER, a
    parse turn of its own; key_table() keeps its thirteen rows; the bit packs next to its neighbours; job_check accepts the key with and
    without "denoise_temporal" in all three modes and still refuses "denoise_temporal" with "noise_threshold" with the text it had; the
    single process and rank 0 set the option, the other ranks do not."""
    src = tmp_path / "key.cpp"
    src.write_text(NATIVE_KEY_TEST)
    exe = str(tmp_path / "key")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(hjr.PKG_DIR, "host"), "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + hjr.PKG_DIR, "-lhenjou_hip", "-Wl,-rpath," + hjr.PKG_DIR, "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "key ok" in p.stdout, p.stdout + p.stderr


def test_render_option_reads_the_key(tmp_path):
    """The key sets bit 24; a file without it parses to the struct it always gave (byte for byte, next to every older key)."""
    load = lambda s: hjr.load_render_option(_option_json(tmp_path, s))
    raw = lambda o: C.string_at(C.addressof(o), C.sizeof(o))
    assert load({"denoise_temporal_response": True}).device_bvh_opt == 1 << 24
    assert load({"denoise_temporal_response": 1, "denoise_temporal": True, "denoise_temporal_moments": True}).device_bvh_opt == (1 << 24) | (1 << 15)
    assert load({"denoise_temporal_response": 1, "denoise_temporal": True}).denoise_variance == 2
    assert load({"denoise_temporal_response": True, "denoise_temporal_coverage": 4, "firefly_clamp": 64, "firefly_clamp_passes": True}).device_bvh_opt == \
        (1 << 24) | (4 << 12) | (64 << 16) | (1 << 23)
    older = {"denoise_temporal": True, "denoise_variance_spatial": True, "denoise_temporal_coverage": 2, "denoise_temporal_moments": True, "firefly_clamp": 8,
             "firefly_clamp_passes": True, "upscale_guided": True, "device_bvh": True, "device_bvh_instances": True, "passes": 4}
    for base in ({}, older):
        for off in (False, 0):
            assert raw(load(dict(base, denoise_temporal_response=off))) == raw(load(base))
        assert load(base).device_bvh_opt & (1 << 24) == 0
        on = load(dict(base, denoise_temporal_response=True))
        assert on.device_bvh_opt == load(base).device_bvh_opt | (1 << 24)
    for bad in (2, -1, "1", 0.5, None):
        with pytest.raises(hjr.HjrError, match="denoise_temporal_response"):
            load({"denoise_temporal_response": bad})


def test_sequence_l_moves_the_light_only():
    """Sequence L: instance 1 of cornelbox.gltf holds the light; it stands for frames 1..3 and then moves by 0.12 per frame in x, the
    inverse consistently; nothing else moves."""
    arrays = Cornell().arrays
    k = light_instance(arrays)
    assert k == 1
    m0, i0 = sequence_transforms(arrays, "L", 3)
    assert np.array_equal(m0, np.asarray(arrays["transforms"], f32).reshape(-1, 12))
    m, inv = sequence_transforms(arrays, "L", 6)
    d = m - m0
    assert np.abs(d[k, 3] - 0.36) < 1e-6 and np.count_nonzero(d) == 1
    p = np.array([0.3, -0.2, 0.7], f32)
    fwd = m[k].reshape(3, 4) @ np.append(p, 1)
    assert np.abs(inv[k].reshape(3, 4) @ np.append(fwd, 1) - p).max() < 1e-5
    assert np.array_equal(sequence_transforms(arrays, "S", 9)[0], m0)


def test_rehearsal_prints_its_table():
    """tools/temporal_response_rehearsal.py at 24 x 16 with references of 64 spp, sequence L: the stages run end to end on the oracle's
    frames.  Frames 1..3 stand still: the change test leaves them nearly alone; frame 4, the first after the light moved, is where it
    answers.  The quality conditions are those of 96 x 64 with 4096 spp references (tests/test_gpu_temporal_response.py):
    printed here, not asserted."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import temporal_response_rehearsal as trr
    from temporal_response_util import format_tables, quality_conditions
    tables, refs = trr.rehearse(Cornell(), 24, 16, 64, sequences="L")
    print(format_tables(tables))
    for text, holds, _ in quality_conditions(tables):
        print("%s: %s (24 x 16: not asserted)" % (text, "holds" if holds else "fails"))
    t = tables["L"]
    assert all(len(t[k]) == 10 and np.isfinite(t[k]).all() for k in ("e_var", "e_tmp", "e_resp", "share"))
    assert t["e_tmp"][0] == t["e_resp"][0] == t["e_var"][0] and t["share"][0] == 0
    assert t["share"][3] > 2 * max(t["share"][1:3]) and t["e_resp"][3] < t["e_tmp"][3]
    assert len(trr.report_worst(t, refs["L"])) == 11
