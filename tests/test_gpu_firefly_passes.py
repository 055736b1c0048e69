"""The firefly clamp on sample passes and adaptive frames on the GPU (option "firefly_clamp_passes"; include/henjou_hip.h "Firefly clamp
on sample passes", DESIGN.md §4 rule 10).

The expectation is numpy float32 (tests/firefly_passes_util.py) on the oracle's chunk sums: after EVERY pass the GPU must give the same
colour bits, the same count of scaled (pixel, chunk) pairs and, on adaptive frames, the same stopped tiles, on both kernel families and
under MIS.  Albedo, normal and variance must not notice the clamp.  Camera at x = 3.5, kappa = 4 throughout (the file-level tests use the
file's camera).  Every prediction is checked not to be vacuous before the GPU is touched."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from firefly_passes_util import oracle_aov_chunks, predict
from firefly_util import f32, firefly_rule, moved_camera
from scene_util import ROOT, Cornell, f32_time, hjr
from test_gpu_adaptive import owned_samples
from test_gpu_progressive import SENTINEL, bits, with_range
from test_gpu_variance import render_var

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
ERR_ARG, ERR_STATE = -1, -5
NEE, MIS = hjr.INTEGRATOR_NEE, hjr.INTEGRATOR_MIS
KAPPA = 4
AOVS = ("colour", "albedo", "normal")


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def cam35(cornell):
    return moved_camera(cornell.camera, 3.5)


@pytest.fixture(scope="module")
def dev(cornell):
    d = cornell.device()
    yield d
    d.close()


@pytest.fixture()
def clamp(dev):
    """Both options on for the test, off after it (and adaptive sampling with them)."""
    dev.set_option("firefly_clamp", KAPPA)
    dev.set_option("firefly_clamp_passes", 1)
    yield dev
    dev.set_adaptive(0.0)
    dev.set_option("firefly_clamp_passes", 0)
    dev.set_option("firefly_clamp", 0)


def params(cornell, cam, w, h, spp, **kw):
    return hjr.make_params(w, h, spp, cam, sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity, **kw)


def same(got, want, what):
    eq = bits(got) == bits(want)
    assert eq.all(), "%s: %d of %d values differ" % (what, int((~eq).sum()), eq.size)


def even_bounds(spp, step):
    return [(b, min(b + step, spp)) for b in range(0, spp, step)]


def run_passes(d, p, bounds, shape):
    """The frame in the given passes through hjr_render_var: per pass ([colour, albedo, normal], variance, stats)."""
    res = []
    for b, e in bounds:
        rc, out, var = render_var(d, with_range(p, b, e), shape)
        assert rc == 0, hjr.lib().hjr_last_error()
        res.append((out, var, d.stats()))
    return res


def check_progressive(cornell, d, cam, w, h, spp, bounds, integ, what):
    """One progressive frame with both options on against the restatement, and against the same passes with "firefly_clamp" 0."""
    chunk, g = oracle_aov_chunks(cornell, w, h, spp, integ, cam)
    pred = predict(chunk, g, w, h, spp, bounds, KAPPA)
    counts = [q["count"] for q in pred]
    print("%s: scaled pairs per pass %s" % (what, counts))
    for (b, e), n in zip(bounds, counts):  # (not vacuous: the rule acts from m_n = 4 on, on some pixels and not on all)
        assert (n > 0) == (e // g >= 4), (e, n)
    p = params(cornell, cam, w, h, spp, integrator=integ)
    d.set_option("firefly_clamp", 0)
    off = run_passes(d, p, bounds, (h, w, 4))
    d.set_option("firefly_clamp", KAPPA)
    on = run_passes(d, p, bounds, (h, w, 4))
    for (b, e), q, (o_off, v_off, st_off), (o_on, v_on, st_on) in zip(bounds, pred, off, on):
        tag = "%s pass [%d, %d)" % (what, b, e)
        same(o_on[0], q["aovs"][0], tag + ": colour vs the restatement")
        assert st_on["firefly_clamped"] == q["count"] and st_off["firefly_clamped"] == 0, (tag, st_on["firefly_clamped"], q["count"])
        same(o_on[1], o_off[1], tag + ": albedo")
        same(o_on[2], o_off[2], tag + ": normal")
        same(v_on, v_off, tag + ": variance")
        same(v_on, q["variance"], tag + ": variance vs the restatement")
        if e // g < 4:
            same(o_on[0], o_off[0], tag + ": colour of a pass the rule does not act on")
    rgb, count, touched = firefly_rule(chunk[:, :, :, 0, :], g, spp, KAPPA)
    d.set_option("firefly_clamp_passes", 0)
    rc, one, one_var = render_var(d, p, (h, w, 4))
    d.set_option("firefly_clamp_passes", 1)
    assert rc == 0 and d.stats()["firefly_clamped"] == count == counts[-1]
    for a, b_, name in zip(on[-1][0] + [on[-1][1]], one + [one_var], AOVS + ("variance",)):
        same(a, b_, what + ": last pass vs the one-shot clamped call, " + name)
    assert (bits(on[-1][0][0]) != bits(off[-1][0][0])).any()
    return counts


@pytest.mark.parametrize("integ, pipeline", [(NEE, 1), (NEE, 2), (MIS, 0)])
def test_progressive_bits(cornell, cam35, integ, pipeline):
    """28 x 20 (ragged tiles), 100 spp (g 8, m 12, r 4) in thirteen passes of 8: NEE on the megakernel and on the wavefront kernels, and
    MIS.  The restatement on the NEE input scales 0, 0, 0, 45, 28, 51, 37, 60, 51, 69, 61, 82 pairs over the first twelve passes and 91
    in the last, which also takes the partial chunk (82 + 9): firefly_rule's count of the one-shot frame."""
    d = cornell.device({"pipeline": pipeline, "firefly_clamp": KAPPA, "firefly_clamp_passes": 1})
    try:
        counts = check_progressive(cornell, d, cam35, 28, 20, 100, even_bounds(100, 8), integ, "integrator %d, pipeline %d" % (integ, pipeline))
        assert d.stats()["pipeline"] == (pipeline - 1 if pipeline else 1)
        if integ == NEE:
            assert counts == [0, 0, 0, 45, 28, 51, 37, 60, 51, 69, 61, 82, 91]
    finally:
        d.close()


def test_uneven_split(cornell, cam35, clamp):
    """[0, 24) [24, 32) [32, 100): a first pass of three chunks, one that brings m_n to exactly 4, and one that ends with the partial chunk."""
    check_progressive(cornell, clamp, cam35, 28, 20, 100, [(0, 24), (24, 32), (32, 100)], NEE, "uneven")


def test_column_length(cornell, cam35, clamp):
    """8 x 8 at 512 spp in passes of 64: m grows to 64, the full 32 KiB LDS column of the kernel."""
    assert hjr.sample_granule(512) == 8
    check_progressive(cornell, clamp, cam35, 8, 8, 512, even_bounds(512, 64), NEE, "512 spp")


# name: (w, h, spp, samples per pass, min_samples, threshold, integrator, rehearsed n_tile histogram, tiles that differ from the raw statistic)
ADAPTIVE = {
    "first": (28, 20, 100, 8, 16, 0.06, NEE, {16: 1, 40: 2, 80: 1, 88: 1, 100: 7}, 2),
    "second": (44, 28, 128, 16, 32, 0.1, NEE, {32: 10, 48: 2, 64: 3, 80: 3, 96: 1, 112: 1, 128: 4}, 7),
    "mis": (28, 20, 100, 8, 16, 0.08, MIS, None, 3),
}
_pred = {}


def adaptive_prediction(cornell, cam, case):
    """(bounds, prediction) of an ADAPTIVE case, checked against the rehearsal and for vacuity on the prediction itself."""
    if case not in _pred:
        w, h, spp, step, ms, thr, integ, hist, differ = ADAPTIVE[case]
        chunk, g = oracle_aov_chunks(cornell, w, h, spp, integ, cam)
        bounds = even_bounds(spp, step)
        pred = predict(chunk, g, w, h, spp, bounds, KAPPA, thr, ms)
        raw = predict(chunk, g, w, h, spp, bounds, KAPPA, thr, ms, stat="raw")
        last = pred[-1]["n_tile"]
        got = {int(v): int((last == v).sum()) for v in np.unique(last)}
        print("%s: n_tile %s, %d tiles differ from the raw statistic, scaled pairs per pass %s"
              % (case, got, int((last != raw[-1]["n_tile"]).sum()), [q["count"] for q in pred]))
        stops = sorted(set(got) - {spp})
        assert len(stops) >= 3, "the prediction stops tiles at %s only" % stops
        assert (last == spp).any(), "the prediction has no tile that never stops"
        assert (last != raw[-1]["n_tile"]).any(), "the clamped statistic decides nothing differently"
        assert int((last != raw[-1]["n_tile"]).sum()) == differ
        assert any(v // g >= 4 for v in stops)  # stops the new kernel decides
        if ms // g < 4:
            assert any(v // g < 4 for v in stops)  # ... and one that is rule 6 as it is
        if hist:
            assert got == hist
        _pred[case] = (bounds, pred)
    return _pred[case]


def run_adaptive(d, p, bounds, shape, pred, what):
    for (b, e), q in zip(bounds, pred):
        rc, out, var = render_var(d, with_range(p, b, e), shape)
        tag = "%s pass [%d, %d)" % (what, b, e)
        assert rc == 0, hjr.lib().hjr_last_error()
        got_n, want_n = d.tile_samples(), owned_samples(q["n_tile"])
        assert (got_n == want_n).all(), "%s: tile_samples\n%s\nwant\n%s" % (tag, got_n, want_n)
        st = d.adaptive_state()
        assert st["owned_tiles"] == want_n.size and st["sample_end"] == e and st["active_tiles"] == q["active"], (tag, st, q["active"])
        for a, w_, name in zip(out, q["aovs"], AOVS):
            same(a, w_, tag + ": " + name)
        same(var, q["variance"], tag + ": variance")
        assert d.stats()["firefly_clamped"] == q["count"], (tag, d.stats()["firefly_clamped"], q["count"])
    assert d.adaptive_state()["samples_rendered"] == 64 * int(owned_samples(pred[-1]["n_tile"]).astype(np.uint64).sum())


@pytest.mark.parametrize("case, pipeline", [("first", 1), ("first", 2), ("second", 1), ("second", 2), ("mis", 0)])
def test_adaptive_tiles_and_aov_bits(cornell, cam35, case, pipeline):
    """After every pass: tile_samples, the active count, all AOV bits, the variance and the counter equal the restatement.
    first: a stop at m_n = 2 (rule 6 as it is), stops at m_n >= 4 (the new kernel's), seven tiles that take the partial chunk."""
    w, h, spp, step, ms, thr, integ, _, _ = ADAPTIVE[case]
    bounds, pred = adaptive_prediction(cornell, cam35, case)
    d = cornell.device({"pipeline": pipeline, "firefly_clamp": KAPPA, "firefly_clamp_passes": 1})
    try:
        d.set_adaptive(thr, ms)
        run_adaptive(d, params(cornell, cam35, w, h, spp, integrator=integ), bounds, (h, w, 4), pred, "%s pipeline %d" % (case, pipeline))
    finally:
        d.close()


def test_shards_give_the_one_rank_frame(cornell, cam35, clamp):
    """The second adaptive input as three packed ranks on one GPU: assembled after every pass they are the one-rank frame (the
    restatement, which test_adaptive_tiles_and_aov_bits holds the one-rank GPU frame to), and their counters add up to its counter."""
    w, h, spp, step, ms, thr, integ, _, _ = ADAPTIVE["second"]
    bounds, pred = adaptive_prediction(cornell, cam35, "second")
    clamp.set_adaptive(thr, ms)
    n_tiles = pred[0]["n_tile"].size
    frames = [[np.zeros((h, w, 4), f32) for _ in range(3)] for _ in bounds]
    tiles = [np.zeros(n_tiles, np.uint32) for _ in bounds]
    counts = [0 for _ in bounds]
    for rank in range(3):
        n = hjr.owned_tiles(w, h, rank, 3)
        p = params(cornell, cam35, w, h, spp, integrator=integ, rank=rank, world_size=3, flags=hjr.FLAG_PACKED)
        for k, (b, e) in enumerate(bounds):
            rc, out, var = render_var(clamp, with_range(p, b, e), (n, 64, 4), variance=False)
            assert rc == 0, hjr.lib().hjr_last_error()
            for a in range(3):
                hjr.unpack_tiles(out[a], frames[k][a], rank, 3)
            tiles[k][rank::3] = clamp.tile_samples()
            counts[k] += clamp.stats()["firefly_clamped"]
    for k, (b, e) in enumerate(bounds):
        for a in range(3):
            same(frames[k][a], pred[k]["aovs"][a], "3 ranks, pass [%d, %d), %s" % (b, e, AOVS[a]))
        assert (tiles[k] == owned_samples(pred[k]["n_tile"])).all()
        assert counts[k] == pred[k]["count"]


def test_device_pointers(cornell, cam35, clamp):
    """hjr_render_device_var into torch tensors on the caller's stream, the first adaptive input: the restatement's bits after every pass."""
    import torch
    w, h, spp, step, ms, thr, integ, _, _ = ADAPTIVE["first"]
    bounds, pred = adaptive_prediction(cornell, cam35, "first")
    clamp.set_adaptive(thr, ms)
    p = params(cornell, cam35, w, h, spp, integrator=integ)
    st = torch.cuda.current_stream().cuda_stream
    for (b, e), q in zip(bounds, pred):
        bufs = [torch.full((h, w, 4), float(SENTINEL), device="cuda") for _ in range(3)]
        var = torch.full((h, w), float(SENTINEL), device="cuda")
        clamp.render_device(with_range(p, b, e), *[t.data_ptr() for t in bufs], stream=st, d_variance=var.data_ptr())
        torch.cuda.synchronize()
        for t, w_, name in zip(bufs, q["aovs"], AOVS):
            same(t.cpu().numpy(), w_, "hjr_render_device_var pass [%d, %d): %s" % (b, e, name))
        same(var.cpu().numpy(), q["variance"], "hjr_render_device_var pass [%d, %d): variance" % (b, e))
        assert (clamp.tile_samples() == owned_samples(q["n_tile"])).all()


def test_render_denoised_filters_the_clamped_pass(cornell, cam35, clamp):
    """hjr_render_denoised in Denoise mode on sample passes = hjr_denoise of the restated pass colour (and the pass's albedo / normal)."""
    w, h, spp = 28, 20, 100
    bounds = [(0, 24), (24, 32), (32, 100)]
    chunk, g = oracle_aov_chunks(cornell, w, h, spp, NEE, cam35)
    pred = predict(chunk, g, w, h, spp, bounds, KAPPA)
    plain = predict(chunk, g, w, h, spp, bounds, 0)
    p = params(cornell, cam35, w, h, spp)
    for (b, e), q, q0 in zip(bounds, pred, plain):
        got = clamp.render_denoised(with_range(p, b, e), hjr.MODE_DENOISE)
        same(got, clamp.denoise(hjr.MODE_DENOISE, *q["aovs"]), "Denoise, pass [%d, %d)" % (b, e))
        if q["count"]:
            assert not np.array_equal(got, clamp.denoise(hjr.MODE_DENOISE, *q0["aovs"]))


def test_state_rules(cornell, cam35, dev):
    """Setting either option between two passes ends the progressive frame: the continuing pass is HJR_ERR_STATE and leaves its outputs
    untouched.  With "firefly_clamp_passes" off the refusal of a pass with "firefly_clamp" on is what it always was."""
    w, h, spp = 20, 12, 64
    p = params(cornell, cam35, w, h, spp)
    try:
        for start, key, value in (((4, 1), "firefly_clamp", 2), ((4, 1), "firefly_clamp", 0), ((4, 1), "firefly_clamp_passes", 1),
                                  ((0, 1), "firefly_clamp", 4), ((0, 0), "firefly_clamp_passes", 1)):
            dev.set_option("firefly_clamp", start[0])
            dev.set_option("firefly_clamp_passes", start[1])
            rc, out, var = render_var(dev, with_range(p, 0, 16), (h, w, 4))
            assert rc == 0, hjr.lib().hjr_last_error()
            dev.set_option(key, value)
            rc, out, var = render_var(dev, with_range(p, 16, 32), (h, w, 4))
            assert rc == ERR_STATE and b"no progressive frame" in hjr.lib().hjr_last_error(), (start, key, value, rc, hjr.lib().hjr_last_error())
            assert all((a == SENTINEL).all() for a in out) and (var == SENTINEL).all()
        dev.set_option("firefly_clamp", KAPPA)
        dev.set_option("firefly_clamp_passes", 0)
        rc, out, var = render_var(dev, with_range(p, 0, 16), (h, w, 4))
        assert rc == ERR_ARG and b"takes whole-frame renders only" in hjr.lib().hjr_last_error()
        assert all((a == SENTINEL).all() for a in out) and (var == SENTINEL).all()
        for bad in (2, -2):
            with pytest.raises(hjr.HjrError, match="firefly_clamp_passes"):
                dev.set_option("firefly_clamp_passes", bad)
    finally:
        dev.set_option("firefly_clamp_passes", 0)
        dev.set_option("firefly_clamp", 0)


def test_whole_frame_render_is_the_one_shot_path(cornell, cam35, dev):
    """With both options on a whole-frame render (sample_end 0, or [0, spp)) is the clamped frame of "firefly_clamp" alone: every AOV, the
    variance and the counter; and "firefly_clamp_passes" without "firefly_clamp" is the plain frame."""
    w, h, spp = 28, 20, 100
    p = params(cornell, cam35, w, h, spp)
    try:
        rc, plain, plain_var = render_var(dev, p, (h, w, 4))
        dev.set_option("firefly_clamp", KAPPA)
        rc, want, want_var = render_var(dev, p, (h, w, 4))
        n = dev.stats()["firefly_clamped"]
        assert rc == 0 and n > 0
        dev.set_option("firefly_clamp_passes", 1)
        for q in (p, with_range(p, 0, spp)):
            rc, out, var = render_var(dev, q, (h, w, 4))
            assert rc == 0 and dev.stats()["firefly_clamped"] == n
            for a, b_, name in zip(out + [var], want + [want_var], AOVS + ("variance",)):
                same(a, b_, "whole frame, both options on, " + name)
        dev.set_option("firefly_clamp", 0)
        for bounds in ([(0, 0)], [(0, 48), (48, 100)]):
            for b, e in bounds:
                rc, out, var = render_var(dev, with_range(p, b, e), (h, w, 4))
                assert rc == 0 and dev.stats()["firefly_clamped"] == 0
            for a, b_, name in zip(out + [var], plain + [plain_var], AOVS + ("variance",)):
                same(a, b_, "firefly_clamp 0, " + name)
    finally:
        dev.set_option("firefly_clamp_passes", 0)
        dev.set_option("firefly_clamp", 0)


def cli_job(tmp_path, section):
    """A 64 x 40 x 64 spp job directory; returns (work dir, run(name, args) -> PNG bytes of frame 1)."""
    assert os.path.exists(CLI), "henjou_cli is not built"
    work = tmp_path / "run"
    shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Image"].update(image_width=64, image_height=40, max_spp=64)
    ro["Animation"].update(start_frame=1, end_frame=2)
    (work / "fps.txt").write_text("24")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")

    def run(name, args, sec=section):
        ro["Image"]["image_name"] = name
        ro["Henjou_HIP"] = sec
        (work / "render_option.json").write_text(json.dumps(ro))
        q = subprocess.run([CLI, "render_option.json"] + args, cwd=work, capture_output=True, text=True, timeout=300, env=env)
        assert q.returncode == 0, q.stdout + q.stderr
        return (work / (name + "_001.png")).read_bytes()
    return work, run


def test_cli_passes_write_the_one_shot_clamped_png(tmp_path):
    """henjou_cli with "firefly_clamp": 4, "firefly_clamp_passes": true, "passes": 4 writes the PNG of "firefly_clamp": 4 alone, byte for
    byte; the rank path as a world of one writes the same bytes.  (That PNG is not the plain frame's: tests/test_gpu_firefly.py.)"""
    work, run = cli_job(tmp_path, {"seed": 3, "firefly_clamp": 4, "firefly_clamp_passes": True, "passes": 4})
    one = run("one", [], {"seed": 3, "firefly_clamp": 4})
    assert run("single", []) == one
    assert run("rank", ["--rank", "0", "--world", "1"]) == one


def test_cli_adaptive_writes_the_python_adaptive_png(tmp_path):
    """... and with "noise_threshold" the PNG of the Python adaptive frame with both options on, on both paths."""
    thr, ms = 0.1, 16
    work, run = cli_job(tmp_path, {"seed": 3, "firefly_clamp": 4, "firefly_clamp_passes": True, "passes": 4, "noise_threshold": thr, "min_samples": ms})
    single = run("single", [])
    assert run("rank", ["--rank", "0", "--world", "1"]) == single
    cwd = os.getcwd()
    os.chdir(work)
    try:
        opt = hjr.load_render_option("render_option.json")
        sc = hjr.Scene(opt.gltf_path.decode(), opt.gltf_name.decode(), opt)
    finally:
        os.chdir(cwd)
    t = f32_time(1, opt.fps)
    arrays = sc.arrays(t)
    d = hjr.Device(0)
    try:
        d.upload_scene(sc.view)
        d.set_transforms(arrays["transforms"], arrays["inv_transforms"])
        p = hjr.make_params(64, 40, 64, sc.camera(opt, t), frame=1, seed=3, sky=tuple(opt.scene_sky_default), ibl_intensity=opt.IBL_intensity)
        d.set_option("firefly_clamp", 4)
        d.set_option("firefly_clamp_passes", 1)
        d.set_adaptive(thr, ms)
        frames = list(d.render_adaptive(p, 4, want_aovs=False))
        n = d.tile_samples()
        assert len(set(n.tolist())) >= 2, n
        d.set_adaptive(0.0)
        d.set_option("firefly_clamp_passes", 0)
        one = d.render(p, want_aovs=False)[0]
    finally:
        d.close()
    got = hjr.load_png(str(work / "single_001.png"))
    assert np.array_equal(got, hjr.float4_to_srgb8(frames[-1][1])[::-1])
    assert not np.array_equal(got, hjr.float4_to_srgb8(one)[::-1])
