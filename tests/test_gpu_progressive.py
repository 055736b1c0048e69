"""A frame rendered in sample passes (hjr_params.sample_begin / sample_end) on the GPU.

The pass that ends at spp must give the one-shot frame's bits for every layout, kernel family, integrator, AOV, shard and fast-math
launch; an intermediate pass must give the running mean that the oracle's per-sample values, summed in the documented order, give;
the counters of the passes must add up to the one-shot launch's; a pass that does not continue the frame is refused without touching
its outputs; and the file-level paths ("Henjou_HIP": {"passes": N}) must write the same PNG bytes.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from scene_util import ROOT, Cornell, hjr

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
SENTINEL = np.float32(-12345.5)
ERR_ARG, ERR_STATE = -1, -5


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


def bits(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what):
    for name, g, w in zip(("color", "albedo", "normal"), got, want):
        if w is None:
            assert g is None, what
            continue
        same = bits(g) == bits(w)
        assert same.all(), "%s, %s: %d of %d values differ" % (what, name, int((~same).sum()), same.size)


def with_range(p, begin, end):
    q = hjr.ParamsV2.from_buffer_copy(p)
    q.sample_begin, q.sample_end = begin, end
    return q


def render_raw(dev, p, shape, aovs=True):
    """hjr_render into sentinel-filled host arrays: (status, [color, albedo, normal])."""
    out = [np.full(shape, SENTINEL, np.float32)] + [np.full(shape, SENTINEL, np.float32) if aovs else None for _ in range(2)]
    rc = hjr.lib().hjr_render(dev._h, C.byref(p), *[None if a is None else a.ctypes.data for a in out])
    return rc, out


def passes(dev, p, bounds, shape, aovs=True):
    """The frame in the given passes; returns the outputs of every pass."""
    res = []
    for b, e in bounds:
        rc, out = render_raw(dev, with_range(p, b, e), shape, aovs)
        assert rc == 0, hjr.lib().hjr_last_error()
        res.append(out)
    return res


def one_shot(dev, p, shape, aovs=True):
    rc, out = render_raw(dev, p, shape, aovs)
    assert rc == 0, hjr.lib().hjr_last_error()
    return out


UNEVEN = [(0, 8), (8, 24), (24, 64)]


@pytest.mark.parametrize("layout", ["lds", "memory", "device_bvh"])
def test_last_pass_equals_one_shot_every_kernel(cornell, layout):
    """Bundled scene on its LDS layout, forced onto the memory layout, and device-built; both kernel families (pipeline 1 / 2); NEE,
    Pathtrace and MIS; uneven passes [0, 8) [8, 24) [24, 64) at 64 spp: the last pass equals the one-shot frame in all three AOVs."""
    opts = {"lds": {}, "memory": {"bvh_width": 4, "lds_bvh": 0}, "device_bvh": {"device_bvh": 1}}[layout]
    dev = cornell.device(opts)
    want_mode = {"lds": (1, 2), "memory": (0,), "device_bvh": (0,)}[layout]
    shape = (40, 48, 4)
    for pipeline in (1, 2):
        dev.set_option("pipeline", pipeline)
        for integ in (hjr.INTEGRATOR_NEE, hjr.INTEGRATOR_PT, hjr.INTEGRATOR_MIS):
            p = cornell.hjr_params(48, 40, 64, integrator=integ)
            ref = one_shot(dev, p, shape)
            st = dev.stats()
            assert st["lds_mode"] in want_mode
            got = passes(dev, p, UNEVEN, shape)
            assert_same(got[-1], ref, "%s pipeline %d integrator %d" % (layout, pipeline, integ))
            assert dev.stats()["pipeline"] == st["pipeline"]


def test_last_pass_equals_one_shot_partial_chunk_and_granule_16(cornell):
    """100 spp (last chunk of 4 samples) ending at 100, and 1024 spp (granule 16) on a small frame."""
    dev = cornell.device()
    shape = (24, 32, 4)
    p = cornell.hjr_params(32, 24, 100)
    ref = one_shot(dev, p, shape)
    for bounds in ([(0, 32), (32, 64), (64, 100)], [(0, 96), (96, 100)], [(0, 8), (8, 100)]):
        assert_same(passes(dev, p, bounds, shape)[-1], ref, "100 spp %s" % bounds)
    assert hjr.sample_granule(1024) == 16
    shape = (16, 16, 4)
    p = cornell.hjr_params(16, 16, 1024)
    ref = one_shot(dev, p, shape)
    assert_same(passes(dev, p, [(0, 16), (16, 512), (512, 1024)], shape)[-1], ref, "1024 spp")
    with pytest.raises(hjr.HjrError, match="multiples"):
        dev.render(with_range(p, 0, 8))


def test_last_pass_equals_one_shot_packed_shard(cornell):
    """Rank 1 of 3, HJR_FLAG_PACKED: [owned tile][64] float4 buffers, the last pass equals the one-shot shard."""
    dev = cornell.device()
    w, h = 40, 24
    n = hjr.owned_tiles(w, h, 1, 3)
    shape = (n, 64, 4)
    p = cornell.hjr_params(w, h, 48, rank=1, world_size=3, flags=hjr.FLAG_PACKED)
    ref = one_shot(dev, p, shape)
    got = passes(dev, p, [(0, 16), (16, 40), (40, 48)], shape)
    assert_same(got[-1], ref, "packed rank 1 of 3")
    full = one_shot(dev, cornell.hjr_params(w, h, 48), (h, w, 4))
    assert_same([hjr.pack_tiles(full[0], 1, 3)], [ref[0]], "packed shard vs full frame")


def test_last_pass_equals_one_shot_fast_math(cornell):
    """A HJR_FLAG_FAST_MATH frame in passes equals the one-shot FAST_MATH frame (not the exact one)."""
    dev = cornell.device()
    shape = (32, 32, 4)
    p = cornell.hjr_params(32, 32, 64, flags=hjr.FLAG_FAST_MATH)
    ref = one_shot(dev, p, shape)
    assert dev.stats()["fast_math"] == 1
    assert_same(passes(dev, p, [(0, 24), (24, 40), (40, 64)], shape)[-1], ref, "fast math")
    assert dev.stats()["fast_math"] == 1


def test_intermediate_passes_equal_oracle_running_mean(cornell):
    """24 x 16 at 48 spp: after each pass the AOVs are the running mean of the oracle's per-sample values, summed in chunks of 8 in
    sample order from 0, the chunk sums in chunk order from +0.0f, times 1 / sample_end.  The test's arithmetic is checked first: at
    sample_end == spp it reproduces the oracle's render."""
    w, h, spp = 24, 16, 48
    osc = ob.OracleScene(cornell.arrays, ob.MATH_PORTABLE)
    op = cornell.oracle_params(w, h, spp)
    chunk = np.zeros((spp // 8, h, w, 3, 3), np.float32)  # [chunk][y][x][aov][rgb]
    for y in range(h):
        for x in range(w):
            for k in range(spp // 8):
                acc = np.zeros((3, 3), np.float32)
                for s in range(8 * k, 8 * k + 8):
                    acc = acc + np.stack(osc.sample(op, x, y, s))
                chunk[k, y, x] = acc

    def running_mean(end):
        run = np.zeros((h, w, 3, 3), np.float32)
        for k in range(end // 8):
            run = run + chunk[k]
        img = run * (np.float32(1) / np.float32(end))
        out = np.ones((3, h, w, 4), np.float32)
        out[..., :3] = np.moveaxis(img, 2, 0)
        return list(out)

    oc, oa, on, _ = osc.render(op)
    assert_same(running_mean(spp), [oc, oa, on], "test arithmetic vs oracle render")
    dev = cornell.device()
    bounds = [(0, 8), (8, 24), (24, 40), (40, 48)]
    got = passes(dev, cornell.hjr_params(w, h, spp), bounds, (h, w, 4))
    for (b, e), out in zip(bounds, got):
        assert_same(out, running_mean(e), "pass [%d, %d)" % (b, e))
    # the generator form yields the same running means
    for (e, c, a, n), out in zip(dev.render_progressive(cornell.hjr_params(w, h, spp), 6), [running_mean(8 * i) for i in range(1, 7)]):
        assert_same([c, a, n], out, "render_progressive sample_end %d" % e)


@pytest.mark.parametrize("integ", [hjr.INTEGRATOR_NEE, hjr.INTEGRATOR_MIS])
def test_pass_counters_add_up(cornell, integ):
    """HJR_FLAG_STATS passes: samples, closest_rays, shadow_rays, shaded_hits, light_samples and nan_samples summed over the passes equal
    the one-shot counting launch's (box / triangle tests depend on scheduling and are left out)."""
    keys = ("samples", "closest_rays", "shadow_rays", "shaded_hits", "light_samples", "nan_samples")
    dev = cornell.device()
    shape = (32, 32, 4)
    p = cornell.hjr_params(32, 32, 64, integrator=integ, flags=hjr.FLAG_STATS)
    ref = one_shot(dev, p, shape)
    one = dev.stats()
    assert one["samples"] == 32 * 32 * 64
    tot = dict.fromkeys(keys, 0)
    for b, e in UNEVEN:
        rc, out = render_raw(dev, with_range(p, b, e), shape)
        assert rc == 0
        st = dev.stats()
        assert st["samples"] == 32 * 32 * (e - b)
        for k in keys:
            tot[k] += st[k]
    assert tot == {k: one[k] for k in keys}
    assert_same(out, ref, "counting passes")
    # STATS may change from pass to pass
    plain = cornell.hjr_params(32, 32, 64, integrator=integ)
    passes(dev, plain, [(0, 8)], shape)
    assert_same(passes(dev, p, [(8, 64)], shape)[-1], ref, "STATS switched on in the second pass")


def test_refused_passes_leave_outputs_and_frame_untouched(cornell):
    """Bad ranges are HJR_ERR_ARG; a gap, a repeated pass, a changed camera / frame / AOV set and new transforms are HJR_ERR_STATE.
    Each refusal leaves the sentinel in the outputs, and the correct next pass still completes the frame bit for bit."""
    dev = cornell.device()
    shape = (24, 32, 4)
    L = hjr.lib()
    p = cornell.hjr_params(32, 24, 64)
    ref = one_shot(dev, p, shape)

    def refused(q, code, words, aovs=True):
        rc, out = render_raw(dev, q, shape, aovs)
        assert rc == code, (rc, L.hjr_last_error())
        msg = L.hjr_last_error().decode()
        assert words in msg, msg
        for a in out:
            if a is not None:
                assert (bits(a) == bits(np.full(shape, SENTINEL, np.float32))).all(), "a refused call wrote its output"

    for b, e in ((0, 12), (4, 16), (8, 8), (16, 8), (0, 72), (56, 65)):
        refused(with_range(p, b, e), ERR_ARG, "sample pass")
    refused(with_range(cornell.hjr_params(32, 24, 8), 0, 4), ERR_ARG, "single chunk")
    refused(with_range(p, 8, 16), ERR_STATE, "no progressive frame")
    passes(dev, p, [(0, 8), (8, 16)], shape)
    refused(with_range(p, 24, 32), ERR_STATE, "does not continue")  # a gap
    refused(with_range(p, 8, 16), ERR_STATE, "does not continue")   # the previous pass again
    moved = cornell.hjr_params(32, 24, 64)
    moved.camera.pos[0] += 0.25
    refused(with_range(moved, 16, 24), ERR_STATE, "camera")
    refused(with_range(cornell.hjr_params(32, 24, 64, frame=2), 16, 24), ERR_STATE, "frame differs")
    refused(with_range(p, 16, 24), ERR_STATE, "AOVs", aovs=False)
    # a commit of unchanged transforms keeps the frame data: the frame goes on
    dev.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
    got = passes(dev, p, [(16, 40), (40, 64)], shape)
    assert_same(got[-1], ref, "after the refusals")
    # the last pass closed the frame
    refused(with_range(p, 64 - 8, 64), ERR_STATE, "no progressive frame")
    # new transforms between two passes: refused, and a new frame started afterwards on the old transforms is the one-shot frame
    passes(dev, p, [(0, 8)], shape)
    m = np.array(cornell.arrays["transforms"], np.float32).reshape(-1, 12).copy()
    inv = np.array(cornell.arrays["inv_transforms"], np.float32).reshape(-1, 12).copy()
    m[:, 3] += 0.5
    inv[:, 3] -= 0.5
    dev.set_transforms(m, inv)
    refused(with_range(p, 8, 16), ERR_STATE, "frame data")
    dev.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
    refused(with_range(p, 8, 16), ERR_STATE, "frame data")
    assert_same(passes(dev, p, UNEVEN, shape)[-1], ref, "restarted frame")
    # a whole-frame render ends an unfinished progressive frame
    passes(dev, p, [(0, 8)], shape)
    one_shot(dev, p, shape)
    refused(with_range(p, 8, 16), ERR_STATE, "no progressive frame")


@pytest.mark.parametrize("mode", [hjr.MODE_DENOISE, hjr.MODE_DENOISE_UPSCALE2X])
def test_denoised_last_pass_equals_one_shot(cornell, mode):
    """hjr_render_denoised in passes filters the running mean; the last pass equals the one-shot call bit for bit."""
    dev = cornell.device()
    p = cornell.hjr_params(32, 32, 64)
    ref = dev.render_denoised(p, mode)
    outs = [dev.render_denoised(with_range(p, b, e), mode) for b, e in UNEVEN]
    assert (bits(outs[-1]) == bits(ref)).all()
    assert not (bits(outs[0]) == bits(ref)).all()  # an intermediate pass is a preview of fewer samples


def _cli_run(tmp_path, name, extra, args):
    work = tmp_path / "run"
    if not work.exists():
        shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
        shutil.copytree(os.path.join(hjr.ASSETS, "LUT"), work / "LUT")
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Image"]["image_name"] = name
    if extra is not None:
        ro["Henjou_HIP"] = extra
    (work / "render_option.json").write_text(json.dumps(ro))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    q = subprocess.run([CLI, "render_option.json"] + args, cwd=work, capture_output=True, text=True, timeout=300, env=env)
    assert q.returncode == 0, q.stdout + q.stderr
    return (work / (name + "_001.png")).read_bytes(), q.stderr


def test_file_level_passes_write_the_same_png(tmp_path):
    """render_option_c1.json (256 x 256 x 16: two chunks) with "passes": 4 renders 2 passes and writes the bytes the config without the
    key writes: through hjr_render_file (henjou_cli's single-GPU path) and through the rank path of henjou_cli."""
    assert os.path.exists(CLI), "henjou_cli is not built"
    base, err0 = _cli_run(tmp_path, "one", None, [])
    assert "sample passes" not in err0
    four, err = _cli_run(tmp_path, "four", {"passes": 4}, [])
    assert "2 sample passes" in err, err
    assert four == base
    rank, err = _cli_run(tmp_path, "rank", {"passes": 4}, ["--rank", "0", "--world", "1"])
    assert "2 sample passes" in err, err
    assert rank == base
    # hjr_render_file through the Python surface
    ro = json.load(open(tmp_path / "run" / "render_option.json"))
    ro["Image"]["image_name"] = "file"
    ro["Henjou_HIP"] = {"passes": 64}
    (tmp_path / "run" / "render_option.json").write_text(json.dumps(ro))
    cwd = os.getcwd()
    os.chdir(tmp_path / "run")
    try:
        hjr.Renderer(0).initializeAndRender("render_option.json")
    finally:
        os.chdir(cwd)
    assert (tmp_path / "run" / "file_001.png").read_bytes() == base
