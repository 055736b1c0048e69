"""The firefly clamp on sample passes without a GPU (option "firefly_clamp_passes"; include/henjou_hip.h "Firefly clamp on sample passes",
DESIGN.md §4 rule 10): properties of the numpy float32 restatement (tests/firefly_passes_util.py), the file key, the file-level refusals,
which come before any device call, and what the rule buys on the CPU oracle."""
import json
import os

import numpy as np
import pytest

from firefly_passes_util import clamped_statistic, pass_rule, predict, samples_share
from firefly_util import f32, firefly_rule, moved_camera, oracle_color_chunks, plain_sum
from scene_util import Cornell, hjr
from test_firefly_host import bits, synthetic

ERR_ARG = -1
NEE = hjr.INTEGRATOR_NEE


def spiked(n, w, h, seed):
    """[n, h, w, 1, 3] chunk sums with a firefly in every tenth pixel or so, in any chunk (the partial last one included)."""
    c = synthetic(n, w * h, seed)
    rng = np.random.default_rng(seed + 1)
    for p in rng.choice(w * h, max(1, w * h // 10), replace=False):
        c[rng.integers(n), p] *= f32(rng.integers(20, 400))
    return c.reshape(n, h, w, 1, 3)


SPLITS = {
    100: [[(0, 100)], [(b, min(b + 8, 100)) for b in range(0, 100, 8)], [(0, 24), (24, 32), (32, 100)], [(0, 96), (96, 100)], [(0, 40), (40, 100)]],
    64: [[(b, b + 8) for b in range(0, 64, 8)], [(0, 8), (8, 56), (56, 64)], [(0, 32), (32, 64)]],
}


@pytest.mark.parametrize("spp", [100, 64])
def test_last_pass_is_the_one_shot_rule_for_any_split(spp):
    """Whatever the passes, the one that ends at spp writes firefly_rule(chunk, g, spp, kappa): colour bits and count."""
    g, w, h = 8, 11, 9
    chunk = spiked((spp + g - 1) // g, w, h, spp)
    want, count, touched = firefly_rule(chunk[:, :, :, 0, :], g, spp, 4)
    assert count > 0 and touched.any() and (~touched).any()
    for bounds in SPLITS[spp]:
        last = predict(chunk, g, w, h, spp, bounds, 4)[-1]
        assert np.array_equal(bits(last["aovs"][0][..., :3]), bits(want)), bounds
        assert last["count"] == count and last["active"] == 4  # (2 x 2 tiles; no stop decisions)


def test_passes_below_four_chunks_are_the_plain_running_mean():
    """m_n < 4: the plain pass's bits and a count of 0; from m_n = 4 on the rule over the received chunks, not over the frame's."""
    g, spp, w, h = 8, 100, 11, 9
    chunk = spiked(13, w, h, 5)
    col = chunk[:, :, :, 0, :]
    bounds = [(b, min(b + 8, spp)) for b in range(0, spp, 8)]
    on, off = predict(chunk, g, w, h, spp, bounds, 4), predict(chunk, g, w, h, spp, bounds, 0)
    for (b, e), p, q in zip(bounds, on, off):
        k = (e + g - 1) // g
        assert np.array_equal(bits(q["aovs"][0][..., :3]), bits(plain_sum(col[:k]) * (f32(1) / f32(e))))
        assert q["count"] == 0 and np.array_equal(bits(p["variance"]), bits(q["variance"]))
        if e // g < 4:
            assert p["count"] == 0 and np.array_equal(bits(p["aovs"][0]), bits(q["aovs"][0])), e
        else:
            rgb, count, touched = pass_rule(col, g, spp, e, 4)
            assert np.array_equal(bits(p["aovs"][0][..., :3]), bits(rgb)) and p["count"] == count
            assert np.array_equal(bits(p["aovs"][0][..., :3])[~touched], bits(q["aovs"][0][..., :3])[~touched]), "a pixel with no scaled chunk moved"
    assert any(p["count"] > 0 for p in on)


def test_clamped_statistic_is_the_raw_one_where_nothing_is_scaled():
    """s_k = 1.0f for every chunk of a pixel gives y'_k = y_k to the bit: the clamped statistic of such a pixel is rule 6's."""
    c = synthetic(8, 33, 1)
    S1, S2 = clamped_statistic(c, 8, 8, 4)
    y = (c[..., 0] + c[..., 1]) + c[..., 2]
    R1, R2 = np.zeros(33, f32), np.zeros(33, f32)
    for k in range(8):
        R1, R2 = R1 + y[k], R2 + y[k] * y[k]
    assert np.array_equal(bits(S1), bits(R1)) and np.array_equal(bits(S2), bits(R2))
    c2 = synthetic(8, 33, 1, spike=(5, 20, 50.0))
    T1, T2 = clamped_statistic(c2, 8, 8, 4)
    moved = bits(T1) != bits(S1)
    assert moved[20] and moved.sum() == 1 and T2[20] < 50 * S2[20]


def _option_json(tmp_path, section, **top):
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Henjou_HIP"] = section
    for k, v in top.items():
        ro[k].update(v)
    path = tmp_path / "render_option.json"
    path.write_text(json.dumps(ro))
    return str(path)


def test_render_option_reads_the_key(tmp_path):
    """"firefly_clamp_passes" is bit 23 of hjr_render_option.device_bvh_opt, strict bool, and needs "firefly_clamp"; kappa's bits stay."""
    load = lambda s: hjr.load_render_option(_option_json(tmp_path, s))
    assert load({"firefly_clamp": 4, "firefly_clamp_passes": True}).device_bvh_opt == (4 << 16) | (1 << 23)
    assert load({"firefly_clamp": 64, "firefly_clamp_passes": 1}).device_bvh_opt == (64 << 16) | (1 << 23)
    assert load({"firefly_clamp": 4, "firefly_clamp_passes": False}).device_bvh_opt == 4 << 16
    assert load({}).device_bvh_opt == 0
    for section in ({"firefly_clamp_passes": True}, {"firefly_clamp": 0, "firefly_clamp_passes": True}, {"firefly_clamp_passes": False}):  # (present is enough, as for every `needs`)
        with pytest.raises(hjr.HjrError, match='firefly_clamp_passes.*needs "firefly_clamp"'):
            load(section)
    for bad in (2, -1, "1", 0.5):
        with pytest.raises(hjr.HjrError, match="firefly_clamp_passes"):
            load({"firefly_clamp": 4, "firefly_clamp_passes": bad})


@pytest.mark.parametrize("extra, word", [({"passes": 2}, "passes"), ({"noise_threshold": 0.05}, "noise_threshold")])
def test_render_file_accepts_passes_with_the_key(tmp_path, extra, word):
    """hjr_render_file: with the key on "firefly_clamp" goes together with "passes" > 1 and "noise_threshold" (the job goes on to the scene,
    which is missing here); without it, or with it false, the refusal and its text are what they were."""
    missing = {"gltf_filename": "no_such_scene.gltf"}
    path = _option_json(tmp_path, dict({"firefly_clamp": 4, "firefly_clamp_passes": True}, **extra), GLTF_file=missing)
    rc = hjr.lib().hjr_render_file(os.fsencode(path), 0)
    err = hjr.lib().hjr_last_error().decode()
    assert rc != 0 and "firefly_clamp" not in err, err
    texts = []
    for section in ({"firefly_clamp": 4}, {"firefly_clamp": 4, "firefly_clamp_passes": False}):
        path = _option_json(tmp_path, dict(section, **extra), GLTF_file=missing)
        assert hjr.lib().hjr_render_file(os.fsencode(path), 0) == ERR_ARG
        texts.append(hjr.lib().hjr_last_error().decode())
        assert "firefly_clamp" in texts[-1] and word in texts[-1] and "no_such_scene" not in texts[-1]
    assert texts[0] == texts[1]
    assert '"firefly_clamp" cannot be combined with "passes" > 1 or "noise_threshold": the clamp needs every chunk sum of a pixel' in texts[0]


def rmse(a, ref):
    d = a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def test_quality_on_the_oracle():
    """What the rule buys, on the CPU oracle: 48 x 32, NEE, seed 1, 256 spp in passes of 32, min_samples 32, kappa 4; RMSE against 8192 spp
    of seed 7 with rule 9's mask (from x = 3.5 every pixel is in it; asserted).  Prints samples rendered / RMSE of today's adaptive frame
    (raw statistic, plain mean), of the raw statistic with the clamped mean and of the rule (clamped statistic, clamped mean) for both
    cameras.  Asserted at x = 3.5, threshold 0.08, against today's adaptive frame at that threshold: the rule's error is below half of it
    (rehearsed ratio 0.31), it renders fewer samples than the raw statistic (0.599 against 0.797), and its RMSE is at most 1.10 x that
    of the raw statistic with the clamped mean (1.033)."""
    import oracle_binding as ob
    cornell = Cornell()
    w, h, spp, kappa = 48, 32, 256, 4
    bounds = [(b, b + 32) for b in range(0, spp, 32)]
    rows = {}
    for name, cam, thresholds in (("x = 3.5", moved_camera(cornell.camera, 3.5), (0.05, 0.08, 0.10, 0.15)), ("scene's own", cornell.camera, (0.08, 0.10))):
        osc = ob.OracleScene(cornell.arrays, ob.MATH_PORTABLE)
        op = ob.make_params(w, h, 8192, cam.as_dict(), seed=7, sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)
        ref = osc.render(op, want_aovs=False)[0]
        mask = ~((ref[..., :3] >= 3.0).any(-1) | (np.abs(ref[..., :3] - f32(0.8)) < 1e-3).all(-1))
        err = lambda p: rmse(p["aovs"][0][mask], ref[mask])
        col, g = oracle_color_chunks(cornell, w, h, spp, NEE, cam)
        chunk = col[:, :, :, None, :]
        uni = [err(predict(chunk, g, w, h, spp, bounds, k)[-1]) for k in (0, kappa)]
        print("camera %s: mask %.0f %%, uniform 256 spp RMSE plain %.5f, clamped %.5f" % (name, 100.0 * mask.mean(), uni[0], uni[1]))
        for t in thresholds:
            today = predict(chunk, g, w, h, spp, bounds, 0, t, 32)[-1]
            raw = predict(chunk, g, w, h, spp, bounds, kappa, t, 32, stat="raw")[-1]
            rule = predict(chunk, g, w, h, spp, bounds, kappa, t, 32)[-1]
            assert (today["n_tile"] == raw["n_tile"]).all()
            rows[name, t] = [(samples_share(p["n_tile"], spp), err(p)) for p in (today, raw, rule)]
            print("camera %s, threshold %.2f: raw statistic, plain mean %.3f / %.5f; raw statistic, clamped mean %.3f / %.5f; clamped statistic, "
                  "clamped mean %.3f / %.5f" % ((name, t) + tuple(v for r in rows[name, t] for v in r)))
        if name == "x = 3.5":
            assert mask.all()
    (s_today, e_today), (s_raw, e_raw), (s_rule, e_rule) = rows["x = 3.5", 0.08]
    assert s_raw == s_today
    assert e_rule < 0.5 * e_today, (e_rule, e_today)
    assert s_rule < s_raw, (s_rule, s_raw)
    assert e_rule <= 1.10 * e_raw, (e_rule, e_raw)
