"""Host-only parts of the variance AOV / variance-guided filter (hjr_render_var, hjr_denoise_var; DESIGN.md §4 rule 7, §11): sanity of
the native checker the GPU filter is compared with (tests/native/denoise_var_ref.cpp), the "denoise_variance" key of the render option
and the field it appends to hjr_render_option.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from denoise_var_util import UNKNOWN, denoise_var_ref, variance_rule
from scene_util import ROOT, hjr
from test_device_bvh import _option_json

f32 = np.float32
H, W = 24, 40


def _step_image():
    """Two flat halves 0.5 apart in luminance ((r + g) + b: 0.3 -> 0.8), flat guides, alpha a ramp."""
    img = np.zeros((H, W, 4), f32)
    img[:, : W // 2, :3] = f32(0.1)
    img[:, W // 2:, 0] = f32(0.1)
    img[:, W // 2:, 1] = f32(0.35)
    img[:, W // 2:, 2] = f32(0.35)
    img[..., 3] = np.linspace(0, 1, H * W, dtype=f32).reshape(H, W)
    guide = np.zeros((H, W, 4), f32)
    return img, guide


def test_checker_alpha_finite_and_variance_bound():
    rng = np.random.default_rng(11)
    img = rng.uniform(0, 2, (H, W, 4)).astype(f32)
    alb = rng.uniform(0, 1, (H, W, 4)).astype(f32)
    nrm = rng.normal(0, 1, (H, W, 4)).astype(f32)
    var = rng.uniform(0, 0.3, (H, W)).astype(f32) ** 2
    var[3, 5] = UNKNOWN  # one pixel without an estimate among known ones
    for mode in (1, 2):
        out, vout = denoise_var_ref(mode, img, alb, nrm, var)
        assert out.shape == ((H, W, 4) if mode == 1 else (2 * H, 2 * W, 4)) and vout.shape == (H, W)
        assert np.isfinite(out).all() and np.isfinite(vout).all()
        assert (vout >= 0).all() and vout.max() <= var.max()
    out, vout = denoise_var_ref(1, img, alb, nrm, var)
    assert np.array_equal(out[..., 3], img[..., 3]), "alpha is the centre's"
    out0, _ = denoise_var_ref(0, img, alb, nrm, var)
    assert np.array_equal(out0, img), "Default copies"
    # everything UNKNOWN: still finite, and the output variance is at most the input's
    out, vout = denoise_var_ref(1, img, alb, nrm, np.full((H, W), UNKNOWN, f32))
    assert np.isfinite(out).all() and np.isfinite(vout).all() and vout.max() <= UNKNOWN


def test_checker_nan_and_negative_variance_act_as_zero():
    rng = np.random.default_rng(12)
    img = rng.uniform(0, 2, (H, W, 4)).astype(f32)
    guide = np.zeros((H, W, 4), f32)
    var = rng.uniform(0, 0.1, (H, W)).astype(f32)
    zeroed = var.copy()
    bad = var.copy()
    for k, (y, x) in enumerate([(0, 0), (5, 7), (23, 39), (12, 20), (12, 21)]):
        zeroed[y, x] = 0
        bad[y, x] = [np.nan, -1.0, -np.inf, -0.0, np.nan][k]
    a, va = denoise_var_ref(1, img, guide, guide, zeroed)
    b, vb = denoise_var_ref(1, img, guide, guide, bad)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
    big = var.copy()
    big[2, 2] = np.inf  # clamped to 1e30 like UNKNOWN
    unk = var.copy()
    unk[2, 2] = UNKNOWN
    assert np.array_equal(denoise_var_ref(1, img, guide, guide, big)[0], denoise_var_ref(1, img, guide, guide, unk)[0])


def test_checker_step_survives_without_variance_and_blurs_without_estimate():
    img, guide = _step_image()
    out, vout = denoise_var_ref(1, img, guide, guide, np.zeros((H, W), f32))
    # V = 0: the tolerance is eps = 1e-3, a step of 0.5 weighs exp(-500) = 0 across the edge: each half stays flat
    assert np.abs(out[..., :3] - img[..., :3]).max() <= 1e-6
    assert (vout == 0).all()
    out, _ = denoise_var_ref(1, img, guide, guide, np.full((H, W), UNKNOWN, f32))
    # V = UNKNOWN: wc = 1, guides only (flat here): the step is blurred over the 5 passes
    lum = out[..., :3].sum(-1)
    assert abs(lum[H // 2, W // 2 - 1] - 0.3) > 0.1 and abs(lum[H // 2, W // 2] - 0.8) > 0.1
    assert np.all(np.diff(lum[H // 2]) >= -1e-6), "a monotone ramp"


def test_variance_rule_restatement():
    """The numpy restatement used by the GPU tests: fewer than two full chunks -> UNKNOWN; constant chunk sums -> 0; the textbook value."""
    c = np.zeros((4, 2, 3), f32)
    c[:, 0] = [[1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3]]
    c[:, 1] = [[1, 0, 0], [3, 0, 0], [5, 0, 0], [7, 0, 0]]
    assert (variance_rule(c, 8, 1, 8) == UNKNOWN).all() and (variance_rule(c, 8, 0, 8) == UNKNOWN).all()
    v = variance_rule(c, 8, 4, 32)
    assert v[0] == 0
    assert abs(float(v[1]) - np.var([1, 3, 5, 7], ddof=1) / (8 * 32)) < 1e-8  # var(sum of m chunks) / n^2 = m s^2 / (m g n)
    assert variance_rule(c, 8, 2, np.array([16, 24]))[1] == f32(f32(f32(4) / f32(2)) / f32(8 * 24))


def test_render_option_parses_denoise_variance(tmp_path):
    """"Henjou_HIP": {"denoise_variance": true}: off by default, with or without the section."""
    for extra in (None, {"seed": 3}, {"denoise_variance": False}, {"denoise_variance": 0}):
        assert hjr.load_render_option(_option_json(tmp_path, extra)).denoise_variance == 0
    for extra in ({"denoise_variance": True}, {"denoise_variance": 1, "passes": 4}):
        assert hjr.load_render_option(_option_json(tmp_path, extra)).denoise_variance == 1
    assert hjr.load_render_option(_option_json(tmp_path, {"denoise_variance": True})).passes == 1


def test_render_option_struct_shorter_and_longer_round_trips(tmp_path):
    """hjr_render_option grew by denoise_variance at its end: the Python mirror matches the C header, a caller with the previous
    (shorter) struct is not written behind its size, a longer one keeps its extra bytes, and both read the same fields."""
    src = tmp_path / "off.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "henjou_hip.h"
int main(void) { printf("%zu %zu %zu %.9g\\n", offsetof(hjr_render_option, min_samples), offsetof(hjr_render_option, denoise_variance), sizeof(hjr_render_option), (double)HJR_VARIANCE_UNKNOWN); return 0; }
""")
    exe = str(tmp_path / "off")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    v = subprocess.check_output([exe]).decode().split()
    O = hjr.RenderOption
    assert [O.min_samples.offset, O.denoise_variance.offset, C.sizeof(O)] == list(map(int, v[:3]))
    assert O.denoise_variance.offset == O.min_samples.offset + 4 and C.sizeof(O) == O.denoise_variance.offset + 4  # appended at the end
    assert f32(float(v[3])) == UNKNOWN == hjr.VARIANCE_UNKNOWN
    path = _option_json(tmp_path, {"denoise_variance": True, "seed": 9, "min_samples": 40}).encode()
    L = hjr.lib()
    full = hjr.load_render_option(path.decode())
    assert full.denoise_variance == 1 and full.min_samples == 40 and full.seed == 9
    short = O.denoise_variance.offset  # the struct of a caller built before this field
    buf = (C.c_ubyte * (short + 64))()
    C.memset(buf, 0xEE, short + 64)
    C.memmove(buf, C.byref(C.c_uint32(short)), 4)
    assert L.hjr_load_render_option(path, C.byref(buf)) == 0
    assert all(b == 0xEE for b in bytes(buf)[short:]), "bytes behind the caller's struct_size were written"
    got = O.from_buffer_copy(bytes(buf)[:short] + bytes(C.sizeof(O) - short))
    assert got.struct_size == short and got.min_samples == 40 and got.seed == 9 and got.denoise_variance == 0
    n = C.sizeof(O) + 32  # a newer caller: the unknown tail stays as it was
    buf = (C.c_ubyte * n)()
    C.memset(buf, 0xAB, n)
    C.memmove(buf, C.byref(C.c_uint32(n)), 4)
    assert L.hjr_load_render_option(path, C.byref(buf)) == 0
    got = O.from_buffer_copy(bytes(buf)[:C.sizeof(O)])
    assert got.struct_size == n and got.denoise_variance == 1 and got.min_samples == 40
    assert all(b == 0xAB for b in bytes(buf)[C.sizeof(O):])
