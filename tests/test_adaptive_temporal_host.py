"""Host-only parts of adaptive sampling that counts the temporal history (option "adaptive_temporal", hjr_temporal_prior; DESIGN.md §4
rule 11): the numpy restatement of rule 11 against hand-made priors and over random statistics (property (b)), the native checker of the
prior against the accumulation's own checker on synthetic plane frames, the "adaptive_temporal" key of the render option, job_check with and
without it, and henjou_cli's refusal for several ranks.  No GPU needed."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import adaptive_temporal_util as atu
from scene_util import ROOT, hjr
from temporal_util import UNKNOWN, identity_xf, temporal_ref, translated, wall_camera
from test_device_bvh import _option_json
from test_temporal_host import H, W, WALL, frame

f32 = np.float32
ERR_ARG = -1
G = 8


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def statistic(rng, shape, m, noise):
    """(S1, S2) of m chunk luminances around 1.0 x G with relative spread `noise`: float32 sums in chunk order from +0.0f."""
    y = (f32(G) * (f32(1) + f32(noise) * rng.standard_normal((m,) + shape).astype(f32))).astype(f32)
    y = np.maximum(y, f32(0))
    S1 = np.zeros(shape, f32)
    S2 = np.zeros(shape, f32)
    for k in range(m):
        S1 = S1 + y[k]
        S2 = S2 + y[k] * y[k]
    return S1, S2


def prior_of(shape, lp, vp, al):
    p = np.zeros(shape + (4,), f32)
    p[..., 0], p[..., 1], p[..., 2] = lp, vp, al
    return p


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_al_one_is_rule_6_bit_for_bit():
    rng = np.random.default_rng(1)
    S1, S2 = statistic(rng, (8, 8), 4, 0.3)
    e6 = atu.rule6_error(S1, S2, 4, 32)
    for lp, vp in ((0.0, 0.0), (1.0, 1e-6), (np.nan, np.nan), (1e30, -1.0)):
        e, same = atu.rule11_error(S1, S2, G, 32, prior_of((8, 8), lp, vp, 1.0))
        assert (bits(e) == bits(e6)).all() and (bits(same) == bits(e6)).all()
    e, _ = atu.rule11_error(S1, S2, G, 32, None)
    assert (bits(e) == bits(e6)).all()
    # rule 6's expression, by hand on one pixel
    m, n = f32(4), f32(32)
    q = max(m * S2[0, 0] - S1[0, 0] * S1[0, 0], f32(0))
    assert bits(e6[0, 0]) == bits(f32(np.sqrt(f32(q / (m - f32(1)))) / f32(S1[0, 0] + f32(1e-3) * n)))


def test_nan_va_gives_e6_and_the_arithmetic_by_hand():
    rng = np.random.default_rng(2)
    S1, S2 = statistic(rng, (8, 8), 2, 0.3)
    e6 = atu.rule6_error(S1, S2, 2, 16)
    for lp, vp in ((1.0, np.nan), (np.nan, 1e-4), (1.0, -1.0), (np.inf, np.inf)):  # NaN va, NaN la, sqrt of a negative, inf / inf
        e, _ = atu.rule11_error(S1, S2, G, 16, prior_of((8, 8), lp, vp, 0.2))
        assert (bits(e) == bits(e6)).all(), (lp, vp)
    # one pixel by hand, every operation one fp32 operation in the header's order
    lp, vp, al = f32(0.9), f32(2e-4), f32(0.25)
    e, _ = atu.rule11_error(S1, S2, G, 16, prior_of((8, 8), lp, vp, al))
    s1, s2, m, n = S1[3, 5], S2[3, 5], f32(2), f32(16)
    lc = f32(s1 / n)
    q = max(f32(f32(m * s2) - f32(s1 * s1)), f32(0))
    vc = f32(f32(q / f32(m * f32(m - f32(1)))) / f32(f32(G) * n))
    om = f32(f32(1) - al)
    va = f32(f32(f32(om * om) * vp) + f32(f32(al * al) * vc))
    la = f32(lp + f32(f32(lc - lp) * al))
    ea = f32(f32(np.sqrt(va)) / f32(max(la, f32(0)) + f32(1e-3)))
    assert bits(e[3, 5]) == bits(min(ea, e6[3, 5]))


def test_a_long_noiseless_history_stops_earlier():
    """vp = 0 with a history at its floor al = 0.2: the accumulated error is a fifth of the frame's own, so a tile that rule 6 keeps
    active at this threshold stops under rule 11; with al = 1 the tile is rule 6's."""
    rng = np.random.default_rng(3)
    y = (f32(G) * (f32(1) + f32(0.4) * rng.standard_normal((8, 8, 8, 1, 1)).astype(f32))).astype(f32)
    chunk = np.maximum(np.broadcast_to(y, (8, 8, 8, 1, 3)) / f32(3), f32(0)).astype(f32)
    bounds = atu.even_bounds(64, 16)
    lum = float(np.mean(chunk.sum(axis=-1)) / G)
    p6 = atu.predict(chunk, G, 8, 8, 64, bounds, 0.08, 16, None)
    p1 = atu.predict(chunk, G, 8, 8, 64, bounds, 0.08, 16, prior_of((8, 8), lum, 0.0, 1.0))
    p11 = atu.predict(chunk, G, 8, 8, 64, bounds, 0.08, 16, prior_of((8, 8), lum, 0.0, 0.2))
    assert p6[-1]["n_tile"][0, 0] == 64 and len(p6) == 4, "rule 6 never stops this tile"
    assert [q["n_tile"][0, 0] for q in p1] == [q["n_tile"][0, 0] for q in p6]
    assert all((bits(a["sum"]) == bits(b["sum"])).all() for a, b in zip(p1, p6) if a["decided"])
    assert p11[-1]["n_tile"][0, 0] == 16 and len(p11) == 1, "the history stops it at its first decision, and the frame ends there"
    assert (bits(p11[0]["aovs"][0]) == bits(p6[0]["aovs"][0])).all(), "the pass's AOVs do not depend on the decision"
    # a 4 x 4 frame: the 48 out-of-image lanes of its one tile carry e = 0, so the same noise does stop under rule 6 (16 of 64 terms)
    small = atu.predict(chunk[:, :4, :4], G, 4, 4, 64, bounds, 0.08, 16, None)
    assert 0 < small[0]["sum"][0, 0] < p6[0]["sum"][0, 0] and small[-1]["n_tile"][0, 0] < 64


def test_property_b_over_random_statistics():
    """e <= e6 per pixel whatever the prior (hostile values included), so the butterfly's sum is <= rule 6's: float addition is monotone."""
    rng = np.random.default_rng(4)
    worse = 0
    for trial in range(200):
        m = int(rng.integers(2, 9))
        S1, S2 = statistic(rng, (64,), m, float(rng.uniform(0.01, 1.0)))
        pr = prior_of((64,), rng.uniform(0, 3, 64), rng.uniform(0, 0.3, 64) ** 2, rng.choice([0.2, 0.25, 1 / 3, 0.5, 1.0], 64))
        if trial % 10 == 0:
            pr[rng.integers(0, 64, 6), rng.integers(0, 2, 6)] = rng.choice([np.nan, np.inf, -1.0, 1e30, 0.0], 6)
        e, e6 = atu.rule11_error(S1, S2, G, m * G, pr)
        ok = np.isnan(e6) | (e <= e6)
        assert ok.all()
        if not np.isnan(e6).any():
            assert atu.butterfly(e) <= atu.butterfly(e6)
        worse += int((e < e6).sum())
    assert worse > 1000, "the priors do lower the error somewhere (%d pixels)" % worse


# ------------------------------------------------------------------------------------------------------------------ the prior's checker
def geometry_of(side):
    return {k: v for k, v in side.items() if k not in ("color", "variance", "history")}


def test_prior_checker_agrees_with_the_accumulation_checker():
    """tests/native/temporal_prior_ref.cpp against tests/native/temporal_ref.cpp on the synthetic plane frames (identity, a moved camera, a
    moving object that disoccludes): the pixels the accumulation restarts are (0, 0, 1, 0), every other pixel's al is max(1 / h, 0.2) of the
    accumulation's history length, vp its propagated variance with a current variance of 0 and al factored out, lp the luminance the blend
    of a black current frame leaves, undone."""
    cam = wall_camera()
    m, inv = translated(identity_xf(2)[1:], identity_xf(2)[1:], (0.5, 0, 0))
    xf_cur = (np.concatenate([identity_xf(1), m]), np.concatenate([identity_xf(1), inv]))
    pairs = [(frame(cam, [WALL], seed=1, hist=2.0), frame(cam, [WALL], seed=2)),
             (frame(wall_camera(0.0), [WALL], seed=3, hist=5.0), frame(wall_camera(1.0), [WALL], seed=4)),
             (frame(cam, [WALL, (-2.0, 1, 3, -0.5, 0.5)], seed=5, hist=7.0), frame(cam, [WALL, (-2.0, 1, 3, 0.0, 1.0)], xf_cur, seed=6))]
    for i, (prev, cur) in enumerate(pairs):
        black = dict(cur, color=np.zeros((H, W, 4), f32), variance=np.zeros((H, W), f32))
        c, v, h = temporal_ref(prev, black, 12)
        pr = atu.prior_ref(prev, geometry_of(cur), 12)
        restart = h == 1
        assert (pr[restart] == atu.NO_PRIOR).all(), i
        assert (i == 0) == (not restart.any())
        al = np.maximum(f32(1) / h, f32(0.2))[~restart]
        got = pr[~restart]
        assert (bits(got[:, 2]) == bits(al)).all() and (got[:, 3] == 0).all(), i
        om = f32(1) - al
        assert np.allclose(got[:, 1] * (om * om), v[~restart], rtol=1e-5, atol=0), i
        lum = (c[..., 0] + c[..., 1]) + c[..., 2]
        assert np.allclose(got[:, 0] * om, lum[~restart], rtol=1e-4, atol=1e-6), i
    # no previous frame, and an unknown variance in a tap
    assert (atu.prior_ref(None, geometry_of(pairs[0][1]), 12) == atu.NO_PRIOR).all()
    prev, cur = pairs[0]
    prev = dict(prev, variance=prev["variance"].copy())
    prev["variance"][3, 4], prev["variance"][6, 7] = UNKNOWN, np.nan
    pr = atu.prior_ref(prev, geometry_of(cur), 12)
    assert (pr[3, 4] == atu.NO_PRIOR).all() and (pr[6, 7] == atu.NO_PRIOR).all() and (pr[..., 2] < 1).sum() >= H * W - 2 * 4


def test_entry_points_are_declared(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text("""
#include "henjou_hip.h"
int (*host_form)(hjr_ctx*, const hjr_temporal_frame*, const hjr_temporal_frame*, float*) = hjr_temporal_prior;
int (*device_form)(hjr_ctx*, const hjr_temporal_frame*, const hjr_temporal_frame*, void*, void*) = hjr_temporal_prior_device;
int main(void) { return host_form == 0 || device_form == 0; }
""")
    exe = str(tmp_path / "decl")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + hjr.PKG_DIR, "-lhenjou_hip",
                           "-Wl,-rpath," + hjr.PKG_DIR, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.run([exe]).returncode == 0
    L = hjr.lib()
    assert L.hjr_temporal_prior(None, None, None, None) == ERR_ARG
    assert L.hjr_temporal_prior_device(None, None, None, None, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------------------------ the key, job_check, the CLI
NATIVE_KEY_TEST = r"""
#include <cstdio>
#include <string>
#include "render_job.hpp"
int main()
{
    using namespace hjr;
    int seen = 0;
    for (const KeyRow& r : key_rows()) if (std::string(r.key) == "adaptive_temporal") seen++;
    const KeyRow& r = key_row("adaptive_temporal");
    if (seen != 1 || std::string(r.key) != "adaptive_temporal" || r.field != &hjr_render_option::device_bvh_opt || r.enc != ENC_BITS || r.shift != 25 || r.width != 1 ||
        r.read != READ_BOOL || !r.needs || std::string(r.needs) != "denoise_temporal" || r.who != WHO_FILTER) { printf("row\n"); return 1; }
    for (const KeyRow& q : key_rows())
        if (&q != &r && q.field == r.field && q.enc == ENC_BITS && q.shift <= 25 && q.shift + q.width > 25) { printf("bit 25 is taken by %s\n", q.key); return 1; }
    // a parse turn of its own, below the moments row's, which stays the table's last row
    const KeyRow& last = key_rows().back();
    if (std::string(last.key) != "denoise_temporal_moments" || !(r.parse < last.parse)) { printf("rank\n"); return 1; }
    for (const KeyRow& q : key_rows()) if (&q != &r && q.parse == r.parse) { printf("parse turn shared with %s\n", q.key); return 1; }
    if (key_table().size() != 13) { printf("key_table\n"); return 1; }
    hjr_render_option o;
    HJR_INIT(o);
    key_put(o, key_row("denoise_temporal_response"), 1);
    key_put(o, key_row("firefly_clamp"), 64);
    key_put(o, key_row("firefly_clamp_passes"), 1);
    key_put(o, r, 1);
    if (o.device_bvh_opt != ((1 << 24) | (64 << 16) | (1 << 23) | (1 << 25)) || key_get(o, r) != 1 || key_get(o, key_row("denoise_temporal_response")) != 1 ||
        key_get(o, key_row("firefly_clamp")) != 64 || key_get(o, key_row("firefly_clamp_passes")) != 1 || key_get(o, key_row("denoise_temporal_moments")) != 0) { printf("pack\n"); return 1; }
    // job_check: "denoise_temporal" with "noise_threshold" is refused without the key, in the old words, and accepted with it
    for (int mode : { (int)HJR_MODE_DENOISE, (int)HJR_MODE_DENOISE_UPSCALE2X })
        for (int key = 0; key < 2; key++) {
            hjr_render_option p;
            HJR_INIT(p);
            p.render_mode = mode; p.image_width = 16; p.image_height = 8; p.noise_threshold = 0.05f;
            key_put(p, key_row("denoise_temporal"), 1);
            if (key) key_put(p, r, 1);
            Job job;
            std::string text;
            const bool ok = job_check(p, job, text);
            if (ok != (key == 1)) { printf("job_check mode %d key %d: %s\n", mode, key, text.c_str()); return 1; }
            if (!key && text != "\"denoise_temporal\" cannot be combined with \"noise_threshold\": an adaptive frame that stops early never reaches the sample pass that advances the history")
                { printf("text: %s\n", text.c_str()); return 1; }
            if (key && !(job.temporal && job.adaptive)) { printf("job\n"); return 1; }
            std::string mine, other, refusal;
            for_each_option(p, single_process(), [&](const char* k, int v) { mine += std::string(k) + "=" + std::to_string(v) + " "; return 0; });
            for_each_option(p, rank_of_world(1), [&](const char* k, int v) { other += std::string(k) + "=" + std::to_string(v) + " "; return 0; });
            const std::string want = std::string("denoise_variance=1 denoise_temporal=1 ") + (key ? "adaptive_temporal=1 " : "");
            if (mine != want || !other.empty()) { printf("options: [%s] [%s], want [%s]\n", mine.c_str(), other.c_str(), want.c_str()); return 1; }
            if (multi_gpu_refusal(p, refusal) != (key == 1) || (key && refusal.find("adaptive_temporal") == std::string::npos)) { printf("multi\n"); return 1; }
        }
    { // without "noise_threshold" the key changes nothing about the job
        hjr_render_option p;
        HJR_INIT(p);
        p.render_mode = HJR_MODE_DENOISE; p.image_width = 16; p.image_height = 8;
        key_put(p, key_row("denoise_temporal"), 1);
        key_put(p, r, 1);
        Job job;
        std::string text;
        if (!job_check(p, job, text) || job.adaptive) { printf("plain\n"); return 1; }
    }
    printf("key ok\n");
    return 0;
}
"""


def test_file_key_row_packs_and_job_check(tmp_path):
    src = tmp_path / "key.cpp"
    src.write_text(NATIVE_KEY_TEST)
    exe = str(tmp_path / "key")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(hjr.PKG_DIR, "host"), str(src), "-o", exe,
                           "-L" + hjr.PKG_DIR, "-lhenjou_hip", "-Wl,-rpath," + hjr.PKG_DIR, "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "key ok" in p.stdout, p.stdout + p.stderr


def test_render_option_reads_the_key(tmp_path):
    load = lambda s: hjr.load_render_option(_option_json(tmp_path, s))
    o = load({"denoise_temporal": True, "adaptive_temporal": True})
    assert o.device_bvh_opt == 1 << 25 and o.denoise_variance == 2
    assert load({"denoise_temporal": True, "adaptive_temporal": 1, "denoise_temporal_moments": True, "denoise_temporal_response": True}).device_bvh_opt == (1 << 25) | (1 << 15) | (1 << 24)
    for off in (False, 0):
        assert load({"denoise_temporal": True, "adaptive_temporal": off}).device_bvh_opt == 0
    for bad in (2, -1, "1", 0.5, None):
        with pytest.raises(hjr.HjrError, match="adaptive_temporal"):
            load({"denoise_temporal": True, "adaptive_temporal": bad})
    with pytest.raises(hjr.HjrError, match='adaptive_temporal needs "denoise_temporal": true'):
        load({"adaptive_temporal": True})
    with pytest.raises(hjr.HjrError, match="needs"):
        load({"adaptive_temporal": True, "denoise_temporal": False})
    # both bad: the new key's turn comes before the moments key's
    with pytest.raises(hjr.HjrError, match="adaptive_temporal"):
        load({"denoise_temporal": True, "adaptive_temporal": 2, "denoise_temporal_moments": 2})


def job_json(tmp_path, section):
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Render_mode"] = "Denoise"
    ro["Henjou_HIP"] = section
    ro["GLTF_file"]["gltf_filename"] = "no_such_scene.gltf"
    path = tmp_path / "x.json"
    path.write_text(json.dumps(ro))
    return path


def test_drivers_accept_the_pair_with_the_key(tmp_path):
    """hjr_render_file and the rank path of henjou_cli: "denoise_temporal" with "noise_threshold" is job_check's old refusal without the
    key; with it both get past job_check and fail on the scene file, which does not exist (no device is touched)."""
    cli = os.path.join(hjr.PKG_DIR, "henjou_cli")
    base = {"denoise_temporal": True, "noise_threshold": 0.05}
    for key in (False, True):
        path = job_json(tmp_path, dict(base, adaptive_temporal=True) if key else base)
        rc = hjr.lib().hjr_render_file(os.fsencode(str(path)), 0)
        err = hjr.lib().hjr_last_error().decode()
        p = subprocess.run([cli, str(path), "--rank", "0", "--world", "1"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert rc != 0 and p.returncode == 1
        if key:
            assert "no_such_scene" in err and "cannot be combined" not in err and "no_such_scene" in p.stderr and "cannot be combined" not in p.stderr
        else:
            assert rc == ERR_ARG and "never reaches the sample pass that advances the history" in err and "no_such_scene" not in err
            assert "never reaches the sample pass that advances the history" in p.stderr


def test_cli_refuses_the_key_with_several_devices(tmp_path):
    """henjou_cli --devices 2 (and "devices": 2 in the file, and a rank of a world of 2) with the key: one line that names the limit, exit
    1, before a rank is started, the scene is loaded or a device is touched."""
    cli = os.path.join(hjr.PKG_DIR, "henjou_cli")
    want = ('henjou_cli: "adaptive_temporal" cannot be combined with "devices" > 1: every rank takes the stop decisions of its own shard without the temporal history, '
            "which only rank 0 keeps")
    section = {"denoise_temporal": True, "adaptive_temporal": True, "noise_threshold": 0.05}
    path = job_json(tmp_path, section)
    runs = [[cli, str(path), "--devices", "2"], [cli, str(path), "--rank", "1", "--world", "2", "--id-fd", "0"]]
    path2 = tmp_path / "y.json"
    ro = json.loads(path.read_text())
    ro["Henjou_HIP"]["devices"] = 2
    path2.write_text(json.dumps(ro))
    runs.append([cli, str(path2)])
    for cmd in runs:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=60, cwd=tmp_path, stdin=subprocess.DEVNULL)
        assert p.returncode == 1, (cmd, p.returncode, p.stderr[-800:])
        assert p.stderr.splitlines() == [want], (cmd, p.stderr[-800:])
    # one device: no such refusal (the job goes on to the scene file, which does not exist)
    p = subprocess.run([cli, str(path), "--devices", "1"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 1 and "devices" not in p.stderr and "no_such_scene" in p.stderr
