"""Adaptive sampling that counts the temporal history on the GPU (option "adaptive_temporal", hjr_temporal_prior[_device];
csrc/hjr_temporal.hip.h section PRIOR, csrc/hjr_aux.hip.h hjr_adaptive_temporal_kernel, DESIGN.md §4 rule 11).

The prior is compared with the native checker tests/native/temporal_prior_ref.cpp bit for bit.  The stateful path is followed frame by
frame and pass by pass: the numpy restatement (tests/adaptive_temporal_util.py), fed the GPU's own prior and the oracle's chunk sums,
predicts the tile states, the active count and the AOVs of every pass; the AOVs that go into the post stage are checked through it: the
image hjr_render_denoised returns equals the native checker's accumulation of the predicted colour and variance, filtered by hjr_denoise_var
with the predicted albedo and normal.  The bundled box from x = 3.5, 64 spp in passes of 16, min_samples 16."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_temporal_util as atu
from scene_util import ROOT, Cornell, hjr
from temporal_util import UNKNOWN, camera_at, moved_consistent, same_bits, temporal_ref
from test_gpu_adaptive import owned_samples
from test_gpu_progressive import bits, with_range

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
ERR_ARG, ERR_STATE = -1, -5
f32 = np.float32
MODE = hjr.MODE_DENOISE
SPP, STEP, MS = 64, 16, 16
# Chosen on the CPU (adaptive_temporal_util.cpu_sequence + vacuity_counts, the oracle's frames and the native checkers; the GPU's frames
# are the oracle's bits): at 0.08 the static 48 x 32 sequence of frames 1..4 has 34 tiles that stop earlier than under rule 6 and 49 that
# survive their first decision; the moved one (frames 3 and 4 shifted by 20 steps: a band of disoccluded pixels along two image edges) has
# one wholly restarted tile at 48 x 32 and four at 28 x 20, one of which stops before spp.
THR = 0.08
FRAMES = (1, 2, 3, 4)
MOVED = (0, 0, 20, 20)
WANT_COUNTS = {  # (w, h, moved) -> vacuity_counts of the sequence: the rehearsal's figures, which the GPU chain must reproduce
    (48, 32, False): {"earlier": 34, "survive": 49, "restarted": 0, "restarted_stop": 0},
    (48, 32, True): {"earlier": 35, "survive": 48, "restarted": 1, "restarted_stop": 0},
    (28, 20, True): {"earlier": 17, "survive": 19, "restarted": 4, "restarted_stop": 1},
}


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


@pytest.fixture(scope="module")
def cam(cornell):
    return camera_at(cornell, x=3.5)


@pytest.fixture(scope="module")
def aux(cornell):
    """The stateless helper: G-buffers, priors, the filter.  Never renders in sample passes."""
    d = cornell.device()
    yield d
    d.close()


def n_tris(cornell):
    return np.asarray(cornell.arrays["indices"]).size // 3


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    same = bits(got) == bits(want)
    assert same.all(), "%s: %d of %d values differ" % (what, int((~same).sum()), same.size)


def params_of(cornell, cam, w, h, frame, integrator=hjr.INTEGRATOR_NEE, spp=SPP):
    return hjr.make_params(w, h, spp, cam, frame=frame, integrator=integrator, sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)


def temporal_device(cornell, on, threshold=THR, **options):
    d = cornell.device(options or None)
    d.set_option("denoise_temporal", 1)
    if on:
        d.set_option("adaptive_temporal", 1)
    d.set_adaptive(threshold, MS)
    return d


# ------------------------------------------------------------------------------------------------------------------ 1. the prior
_frames = {}


def rendered(cornell, aux, w, h, k, cam, frame, coverage=0):
    """One frame as a side of the accumulation: 24 spp with its variance and the G-buffer from the GPU, instances moved by k steps."""
    key = (w, h, k, bytes(cam), frame, coverage)
    if key not in _frames:
        m, inv = moved_consistent(cornell.arrays, k)
        aux.set_transforms(m, inv)
        p = params_of(cornell, cam, w, h, frame, spp=24)
        c, a, n, v = aux.render(p, want_variance=True)
        _frames[key] = {"camera": cam, "transforms": m, "inv_transforms": inv, "gbuffer": aux.gbuffer(p, coverage), "color": c, "variance": v}
        if coverage:
            _frames[key]["coverage"] = coverage
    return {k2: (v2.copy() if isinstance(v2, np.ndarray) else v2) for k2, v2 in _frames[key].items()}


def geometry_of(side):
    """The current side of a prior: no colour, no variance."""
    return {k: v for k, v in side.items() if k not in ("color", "variance", "history")}


@pytest.mark.parametrize("w,h", [(48, 32), (28, 20)])
@pytest.mark.parametrize("case", ["static", "moved", "camera", "no_prev", "unknown", "coverage2"])
def test_prior_equals_native_checker(cornell, aux, cam, w, h, case):
    """hjr_temporal_prior (host form) and hjr_temporal_prior_device equal tests/native/temporal_prior_ref.cpp bit for bit; the cases have
    the pixels they are about (carried ones with al < 1, restarted ones, unknown ones with (0, 0, 1, 0))."""
    cam1 = camera_at(cornell, x=3.5, turn=0.04, shift=(-0.05, 0.03, 0.06)) if case == "camera" else cam
    k0, k1 = (1, 21) if case == "moved" else (0, 0)
    cov = 2 if case == "coverage2" else 0
    prev = rendered(cornell, aux, w, h, k0, cam, 1, cov)
    prev["history"] = np.random.default_rng(w * h).integers(1, 41, (h, w)).astype(f32)
    cur = geometry_of(rendered(cornell, aux, w, h, k1, cam1, 2, cov))
    if case == "unknown":
        prev["variance"][::5, ::7] = UNKNOWN
        prev["variance"][1, 1] = np.nan
    if case == "no_prev":
        prev = None
    want = atu.prior_ref(prev, cur, n_tris(cornell))
    got = aux.temporal_prior(prev, cur)
    assert_bits(got, want, "%s %dx%d, host form" % (case, w, h))
    none = (want == atu.NO_PRIOR).all(axis=-1)
    carried = want[..., 2] < 1
    assert (none | carried).all() and (want[..., 3] == 0).all()
    if case == "no_prev":
        assert none.all()
    else:
        assert carried.mean() > 0.5, "most pixels find their history (%.0f %%)" % (100 * carried.mean())
        assert (want[carried][:, 2] >= f32(0.2)).all() and (want[carried][:, 2] <= f32(0.5)).all()
    if case in ("moved", "unknown"):
        assert none.sum() >= 16, "the case has pixels without a usable history"
    if case == "unknown":
        assert not np.isnan(want).any()
    # the device form: the same frames through device pointers
    import torch
    keep = []
    to_dev = lambda a: keep.append(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()) or keep[-1].data_ptr()

    def frame_of(d, images):
        f = hjr.Device._temporal_frame(d, keep, images=images)
        f.transforms12, f.inv_transforms12 = to_dev(np.asarray(d["transforms"], f32)), to_dev(np.asarray(d["inv_transforms"], f32))
        f.gbuffer = to_dev(np.ascontiguousarray(d["gbuffer"], hjr.GBUFFER_DTYPE))
        if images:
            f.color, f.variance, f.history = to_dev(np.asarray(d["color"], f32)), to_dev(np.asarray(d["variance"], f32)), to_dev(np.asarray(d["history"], f32))
        return f
    fc = frame_of(cur, False)
    fp = None if prev is None else frame_of(prev, True)
    out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    rc = hjr.lib().hjr_temporal_prior_device(aux._h, None if fp is None else C.byref(fp), C.byref(fc), C.c_void_p(out.data_ptr()), None)
    assert rc == 0, hjr.lib().hjr_last_error()
    aux.synchronize()
    assert_bits(out.cpu().numpy(), want, "%s %dx%d, device form" % (case, w, h))


def test_prior_host_entry_staging_at_an_odd_pixel_count(aux):
    """hjr_temporal_prior through its host entry point at 7 x 5 pixels and 3 instances (temporal_response_util.staging_case: one-float
    images of an odd number of floats in the staging buffer) equals tests/native/temporal_prior_ref.cpp bit for bit."""
    from temporal_response_util import P_TRIS, staging_case
    prev, cur = staging_case()
    prev = {k: v for k, v in prev.items() if k != "moments"}
    want = atu.prior_ref(prev, geometry_of(cur), P_TRIS)
    assert_bits(aux.temporal_prior(prev, geometry_of(cur)), want, "7 x 5, 3 instances, host form")
    assert (want[..., 2] < 1).any(), "pixels are carried: the previous side's images were read"


def test_prior_argument_checks(cornell, aux, cam):
    L = hjr.lib()
    prev = rendered(cornell, aux, 28, 20, 0, cam, 1)
    prev["history"] = np.ones((20, 28), f32)
    cur = geometry_of(rendered(cornell, aux, 28, 20, 0, cam, 2))
    keep = []
    fc = hjr.Device._temporal_frame(cur, keep, images=False)
    out = np.zeros((20, 28, 4), f32)
    assert L.hjr_temporal_prior(aux._h, None, C.byref(fc), None) == ERR_ARG
    assert L.hjr_temporal_prior(aux._h, None, None, out.ctypes.data) == ERR_ARG
    assert L.hjr_temporal_prior(None, None, C.byref(fc), out.ctypes.data) == ERR_ARG
    assert L.hjr_temporal_prior(aux._h, None, C.byref(fc), out.ctypes.data) == 0  # colour and variance of cur are NULL
    fp = hjr.Device._temporal_frame(prev, keep)
    fp.history = None
    assert L.hjr_temporal_prior(aux._h, C.byref(fp), C.byref(fc), out.ctypes.data) == ERR_ARG
    small = {k: (v[:16, :24].copy() if isinstance(v, np.ndarray) and v.shape[:2] == (20, 28) else v) for k, v in prev.items()}
    with pytest.raises(hjr.HjrError):
        aux.temporal_prior(small, cur)  # sizes differ
    fc.gbuffer = None
    assert L.hjr_temporal_prior(aux._h, None, C.byref(fc), out.ctypes.data) == ERR_ARG


# ------------------------------------------------------------------------------------------------------------------ 2. the stateful path
def follow_sequence(cornell, aux, dev, cam, w, h, moved, integrator=hjr.INTEGRATOR_NEE, frames=FRAMES, coverage=0, what=""):
    """Frames `frames` through hjr_render_denoised on `dev` (option on), pass by pass against the restatement; returns the frames as
    adaptive_temporal_util.vacuity_counts takes them."""
    nt = n_tris(cornell)
    bounds = atu.even_bounds(SPP, STEP)
    prev, seq = None, []
    for i, f in enumerate(frames):
        k = moved[i] if moved else 0
        xf = moved_consistent(cornell.arrays, k)
        arrays = dict(cornell.arrays, transforms=xf[0], inv_transforms=xf[1])
        dev.set_transforms(*xf)
        aux.set_transforms(*xf)
        p = params_of(cornell, cam, w, h, f, integrator)
        geom = {"camera": cam, "transforms": xf[0], "inv_transforms": xf[1], "gbuffer": aux.gbuffer(p, coverage)}
        if coverage:
            geom["coverage"] = coverage
        prior = None
        if prev is not None:
            prior = aux.temporal_prior(prev, geom)
            assert_bits(prior, atu.prior_ref(prev, geom, nt), "%s frame %d: the prior" % (what, f))
        chunk, g = atu.oracle_frame_chunks(cornell, arrays, ("moved", k), w, h, SPP, cam, f, integrator)
        pred = atu.predict(chunk, g, w, h, SPP, bounds, THR, MS, prior)
        pred6 = atu.predict(chunk, g, w, h, SPP, bounds, THR, MS, None)
        for q in pred:
            b, e = q["bounds"]
            tag = "%s frame %d pass [%d, %d)" % (what, f, b, e)
            out = dev.render_denoised(with_range(p, b, e), MODE)
            got_n, want_n = dev.tile_samples(), owned_samples(q["n_tile"])
            assert (got_n == want_n).all(), "%s: tile_samples\n%s\nwant\n%s" % (tag, got_n, want_n)
            st = dev.adaptive_state()
            assert st["active_tiles"] == q["active"] and st["sample_end"] == e and st["owned_tiles"] == want_n.size, tag
            cur = dict(geom, color=q["aovs"][0], variance=q["variance"])
            acc = temporal_ref(prev, cur, nt) if not coverage else __import__("temporal_cov_util").temporal_cov_ref(prev, cur, nt)
            assert_bits(out, aux.denoise(MODE, acc[0], q["aovs"][1], q["aovs"][2], variance=acc[1]), tag + ": the filtered accumulation of the predicted AOVs")
        prev = dict(cur, color=acc[0], variance=acc[1], history=acc[2])
        seq.append({"prior": prior, "pred": pred, "pred6": pred6, "geom": geom, "spp": SPP, "step": STEP})
    return seq


@pytest.mark.parametrize("name,w,h,moved,pipeline", [("static-mega", 48, 32, False, 1), ("static-wavefront", 48, 32, False, 2), ("moved", 48, 32, True, 0), ("ragged-moved", 28, 20, True, 0)])
def test_rule_11_equals_the_restatement(cornell, aux, cam, name, w, h, moved, pipeline):
    """After every pass of every frame: tile states, active count, hjr_copy_tile_samples and the AOVs into the post stage equal the numpy
    restatement fed the GPU's prior and the oracle's chunk sums (frame 1 has no history: rule 6, property (a)).  Property (b) and the
    three not-vacuous conditions are counted on the same chain (vacuity_counts asserts (b) and that wholly restarted tiles take rule 6's
    sums bit for bit), and the counts are the CPU rehearsal's."""
    dev = temporal_device(cornell, True)
    try:
        dev.set_option("pipeline", pipeline)
        seq = follow_sequence(cornell, aux, dev, cam, w, h, MOVED if moved else None, what=name)
        assert dev.stats()["pipeline"] == (1 if pipeline == 2 else 0)
    finally:
        dev.close()
    counts = atu.vacuity_counts(seq)
    print(name, counts)
    assert counts == WANT_COUNTS[(w, h, moved)]
    if not moved:
        assert counts["earlier"] >= 1 and counts["survive"] >= 1
    else:
        assert counts["restarted"] >= 1


def test_rule_11_with_mis_and_coverage(cornell, aux, cam):
    """The same chain with the MIS integrator (three frames, 28 x 20) and, on NEE, with "denoise_temporal_coverage" 2: the prior runs the
    coverage instantiation on the coverage G-buffer."""
    dev = temporal_device(cornell, True)
    try:
        seq = follow_sequence(cornell, aux, dev, cam, 28, 20, None, hjr.INTEGRATOR_MIS, frames=(1, 2, 3), what="mis")
        assert atu.vacuity_counts(seq)["earlier"] >= 1
        dev.set_option("denoise_temporal_coverage", 2)
        seq = follow_sequence(cornell, aux, dev, cam, 28, 20, MOVED, frames=(1, 2, 3), coverage=2, what="coverage 2")
        assert any((fr["prior"][..., 2] < 1).any() for fr in seq[1:])
    finally:
        dev.close()


def run_frame(dev, p, stop_early=True):
    """All passes of one frame: [(filtered image, tile_samples, active)]; ends where the driver ends it (no active tile)."""
    out = []
    for b, e in atu.even_bounds(SPP, STEP):
        img = dev.render_denoised(with_range(p, b, e), MODE)
        out.append((img, dev.tile_samples(), dev.adaptive_state()["active_tiles"]))
        if stop_early and out[-1][2] == 0:
            break
    return out


@pytest.mark.parametrize("w,h", [(48, 32), (28, 20)])
def test_property_a_and_b_against_the_option_off(cornell, cam, w, h):
    """Property (a): frame 1, and a frame after hjr_temporal_reset, with the option on equal the option off after every pass: tile
    states, active counts and the filtered image (all AOVs enter it).  Property (b): in the frames with a history every tile's n_tile
    with the option on is <= its n_tile under rule 6 (the option off) on the same frame and passes."""
    on, off = temporal_device(cornell, True), temporal_device(cornell, False)
    try:
        for f in (1, 2, 3):
            p = params_of(cornell, cam, w, h, f)
            if f == 3:
                on.temporal_reset()
                off.temporal_reset()
            a, b = run_frame(on, p), run_frame(off, p)
            if f != 2:
                assert len(a) == len(b)
                for k, ((ia, na, aa), (ib, nb, ab)) in enumerate(zip(a, b)):
                    assert (na == nb).all() and aa == ab, "frame %d pass %d" % (f, k)
                    assert_bits(ia, ib, "frame %d pass %d" % (f, k))
            else:
                assert (a[-1][1] <= b[-1][1]).all() and (a[-1][1] < b[-1][1]).any()
    finally:
        on.close()
        off.close()


# ------------------------------------------------------------------------------------------------------------------ 3. history, state, refusals
def by_hand(aux, cornell, cam, w, h, f, prev, n=STEP):
    """The frame every tile of which stopped at n samples: render of [0, n) with its variance, accumulated against prev by the native
    checker, filtered: (image, the new history)."""
    p = params_of(cornell, cam, w, h, f)
    c, a, nn, v = aux.render(with_range(p, 0, n), want_variance=True)
    cur = {"camera": cam, "transforms": cornell.arrays["transforms"], "inv_transforms": cornell.arrays["inv_transforms"], "gbuffer": aux.gbuffer(p), "color": c, "variance": v}
    tc, tv, th = temporal_ref(prev, cur, n_tris(cornell))
    return aux.denoise(MODE, tc, a, nn, variance=tv), dict(cur, color=tc, variance=tv, history=th)


def test_history_advances_when_the_frame_ends_early(cornell, aux, cam):
    """A threshold every tile meets at its first decision: the frame ends at 16 of 64 spp.  With the option on that pass commits the
    history: frame 2 differs from a restart and equals the checker's blend against frame 1; a pass that continues the committed frame is
    HJR_ERR_STATE.  With the option off the parent's behaviour stands: the history never advances and frame 2 is a restart."""
    w, h = 28, 20
    aux.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
    want1, hist1 = by_hand(aux, cornell, cam, w, h, 1, None)
    want2, _ = by_hand(aux, cornell, cam, w, h, 2, hist1)
    restart2, _ = by_hand(aux, cornell, cam, w, h, 2, None)
    assert not same_bits(want2, restart2)
    L = hjr.lib()
    out = np.zeros((h, w, 4), f32)
    for on in (True, False):
        dev = temporal_device(cornell, on, threshold=1e3)
        try:
            p1, p2 = params_of(cornell, cam, w, h, 1), params_of(cornell, cam, w, h, 2)
            assert_bits(dev.render_denoised(with_range(p1, 0, STEP), MODE), want1, "frame 1")
            assert dev.adaptive_state()["active_tiles"] == 0
            if on:  # the state rule: the frame is over
                assert L.hjr_render_denoised(dev._h, C.byref(with_range(p1, STEP, 2 * STEP)), MODE, out.ctypes.data, w, h) == ERR_STATE
                assert b"adaptive_temporal" in L.hjr_last_error()
            assert_bits(dev.render_denoised(with_range(p2, 0, STEP), MODE), want2 if on else restart2, "frame 2, option %s" % ("on" if on else "off"))
            if on:  # setting the option ends an unfinished progressive frame and keeps the history
                dev.set_adaptive(THR, MS)
                p3 = params_of(cornell, cam, w, h, 3)
                dev.render_denoised(with_range(p3, 0, STEP), MODE)
                dev.set_option("adaptive_temporal", 1)
                assert L.hjr_render_denoised(dev._h, C.byref(with_range(p3, STEP, 2 * STEP)), MODE, out.ctypes.data, w, h) == ERR_STATE
        finally:
            dev.close()


def test_refused_with_an_acting_firefly_clamp_passes(cornell, cam):
    w, h = 28, 20
    L = hjr.lib()
    out = np.zeros((h, w, 4), f32)
    dev = temporal_device(cornell, True)
    try:
        p = with_range(params_of(cornell, cam, w, h, 1), 0, STEP)
        dev.set_option("firefly_clamp", 4)
        dev.set_option("firefly_clamp_passes", 1)
        assert L.hjr_render_denoised(dev._h, C.byref(p), MODE, out.ctypes.data, w, h) == ERR_ARG
        msg = L.hjr_last_error()
        assert b"adaptive_temporal" in msg and b"firefly_clamp_passes" in msg
        assert not out.any(), "nothing was rendered"
        dev.set_option("firefly_clamp", 0)  # kappa 0: rule 10 does not act
        assert L.hjr_render_denoised(dev._h, C.byref(p), MODE, out.ctypes.data, w, h) == 0, L.hjr_last_error()
        with pytest.raises(hjr.HjrError):
            dev.set_option("adaptive_temporal", 2)
        # outside its one situation the option changes nothing: a whole-frame render, Default mode
        off = temporal_device(cornell, False)
        try:
            whole = params_of(cornell, cam, w, h, 1)
            for mode in (MODE, hjr.MODE_DEFAULT):
                assert_bits(dev.render_denoised(whole, mode), off.render_denoised(whole, mode), "whole frame, mode %d" % mode)
                dev.temporal_reset()
                off.temporal_reset()
        finally:
            off.close()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------------------------ 4. file level
def test_cli_two_frame_job(tmp_path):
    """henjou_cli on a two-frame job with the key: both PNGs are written and frame 2, which has a history, renders fewer samples than
    frame 1, which has none."""
    work = tmp_path / "job"
    shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Image"].update(image_width=96, image_height=64, max_spp=64, image_name="at")
    ro["Animation"].update(start_frame=1, end_frame=3)
    ro["Camera"]["camera_position"][0] = 3.5
    ro["Camera"]["allow_camera_animation"] = False
    ro["Render_mode"] = "Denoise"
    ro["Henjou_HIP"] = {"denoise_temporal": True, "adaptive_temporal": True, "noise_threshold": THR, "min_samples": MS, "passes": 4}
    (work / "render_option.json").write_text(json.dumps(ro))
    p = subprocess.run([CLI, "render_option.json"], cwd=work, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    for f in (1, 2):
        assert (work / ("at_%03d.png" % f)).stat().st_size > 0
    n = [int(m) for m in re.findall(r"(\d+) samples rendered", p.stderr)]
    assert len(n) == 2 and n[1] < n[0], p.stderr


# ------------------------------------------------------------------------------------------------------------------ 5. what it buys
def test_quality_and_saving(cornell):
    """The table of tools/adaptive_temporal_bench.py: sequences S and M at 96 x 64, eight frames of 256 spp in passes
    of 32, threshold 0.08, references of 4096 spp.  Asserted: what property (b) guarantees (every tile of every frame receives at most
    rule 6's samples, so no frame renders more samples than the adaptive arm's), and the error against the adaptive-without-temporal arm
    of the same run, mean RMSE of the filtered output over frames 2..8: at most 1.00 x that arm's on S and 1.25 x on M.  The bounds are the
    CPU rehearsal's figures (tools/adaptive_temporal_rehearsal.py at this size: 0.963 and 1.218, the GPU's frames being the oracle's bits)
    with its margin on S dropped and 2.5 % added on M, where the loss is the temporal path's own (its full-spp arm is at 1.194: §11.2's
    frames 3 and 6).  The saving is printed, not asserted: how many samples a history saves is the scene's."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import adaptive_temporal_bench as atb
    res = atb.quality()
    for name, bound in (("S", 1.00), ("M", 1.25)):
        t = res[name]
        assert all(t["property_b"]), "%s: n_tile(on) <= n_tile(rule 6) for every tile of every frame" % name
        assert t["both"]["samples"][0] == t["adaptive"]["samples"][0], "frame 1 has no history"
        assert all(b <= a for a, b in zip(t["adaptive"]["samples"], t["both"]["samples"]))
        e_both, e_ad = float(np.mean(t["both"]["rmse"][1:])), float(np.mean(t["adaptive"]["rmse"][1:]))
        share = sum(t["both"]["samples"][1:]) / sum(t["adaptive"]["samples"][1:])
        print("%s: mean RMSE(2..8) both %.5f, adaptive %.5f (ratio %.3f, bound %.2f); samples of frames 2..8 against the adaptive arm: %.3f" % (name, e_both, e_ad, e_both / e_ad, bound, share))
        assert e_both <= bound * e_ad
