"""Thin-film LUT lookup semantics (disneyBRDF.h:11-14,213-217; sampler state renderer.h:854-898): wrap addressing,
texel-centre offset, bilinear weights, and the effect on the Disney specular F0."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import shading_cases as sc
from scene_util import load_lut

L = ob.lib()


def fetch(lut, u, v):
    o = ob.F3()
    L.hjo_lut_fetch(lut.ctypes.data, lut.shape[1], lut.shape[0], u, v, o)
    return np.array(o, np.float32)


def test_texel_centres_wrap_and_bilinear():
    lut = np.zeros((4, 8, 4), np.uint8)
    lut[..., 0] = np.arange(8)[None, :] * 30
    lut[..., 1] = np.arange(4)[:, None] * 60
    lut[..., 3] = 255
    for i in range(8):
        for j in range(4):
            got = fetch(lut, (i + 0.5) / 8, (j + 0.5) / 4)  # texel centres return the texel (normalised float read)
            assert np.allclose(got[:2], [i * 30 / 255, j * 60 / 255], atol=1e-6)
    mid = fetch(lut, 1.0 / 8 + 0.5 / 8 + 0.5 / 8, 0.5 / 4)  # halfway between texel 1 and 2
    assert np.isclose(mid[0], 0.5 * (30 + 60) / 255, atol=1e-6)
    assert np.allclose(fetch(lut, 0.5 / 8 + 1.0, 0.5 / 4 - 2.0), fetch(lut, 0.5 / 8, 0.5 / 4))  # cudaAddressModeWrap
    edge = fetch(lut, 0.0, 0.5 / 4)  # u = 0 blends the last and first column
    assert np.isclose(edge[0], 0.5 * (0 + 210) / 255, atol=1e-6)


def test_thinfilm_changes_specular_f0():
    lut = load_lut()
    assert lut.shape == (256, 256, 4)
    m = ob.Material()
    m.basecolor = ob.F3(0.35, 0.8, 0.8)
    m.roughness, m.metallic, m.ior = 0.3, 0.0, 1.0
    wo = ob.F3(0.3, 0.9, 0.1)
    wi = ob.F3(-0.25, 0.93, 0.05)
    f0, f1, f2 = ob.F3(), ob.F3(), ob.F3()
    L.hjo_bsdf_eval(ob.MATH_PORTABLE, C.byref(m), wo, wi, None, 0, 0, f0)
    m.is_thinfilm = 1
    L.hjo_bsdf_eval(ob.MATH_PORTABLE, C.byref(m), wo, wi, lut.ctypes.data, 256, 256, f1)
    L.hjo_bsdf_eval(ob.MATH_PORTABLE, C.byref(m), wo, wi, None, 0, 0, f2)  # no LUT bound: F0 = 0
    a, b, c = np.array(f0), np.array(f1), np.array(f2)
    assert not np.allclose(a, b) and not np.allclose(b, c)
    assert len(set(np.round(b, 6))) > 1  # the film tints the highlight: channels differ although base colour y == z


# ------------------------------------------------------------------ the fetch against a float64 restatement, at unlike shapes
def bilinear_f64(table, scale, u, v):
    """The documented sampler rule in float64 for the float32 coordinates (u, v): texel-centre offset x = u * w - 0.5, the weight
    frac(x) rounded to 1/256 (floor(frac * 256 + 0.5) / 256), wrap addressing of both taps, texel * scale, bilinear blend.  table is
    [h, w, >= 3]; returns (rgb, the largest |texel * scale| among the four taps)."""
    h, w = table.shape[:2]
    x, y = float(u) * w - 0.5, float(v) * h - 0.5
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = np.floor((x - fx) * 256.0 + 0.5) / 256.0, np.floor((y - fy) * 256.0 + 0.5) / 256.0
    i0, j0 = int(fx) % w, int(fy) % h  # Python's % is the wrap: never negative
    i1, j1 = (i0 + 1) % w, (j0 + 1) % h
    t = table[..., :3].astype(np.float64) * scale
    out = (1 - ax) * (1 - ay) * t[j0, i0] + ax * (1 - ay) * t[j0, i1] + (1 - ax) * ay * t[j1, i0] + ax * ay * t[j1, i1]
    return out, np.abs([t[j0, i0], t[j0, i1], t[j1, i0], t[j1, i1]]).max()


def clear_of_weight_steps(u, v, w, h):
    """False where a coordinate lies so close to a step of the 1/256 weight rounding that the float32 position u * w - 0.5 (one rounding
    of a product below w: at most w * 2^-24 off) and the float64 one may round to neighbouring weights.  Such points say nothing about
    the fetch; texel centres and texel boundaries are half a step away from every step."""
    for c, n in ((u, w), (v, h)):
        s = (float(c) * n - 0.5) * 256.0 + 0.5
        if abs(s - np.round(s)) < 256.0 * n * 2.0 ** -23:
            return False
    return True


def fetch_points(h, w, seed):
    """(u, v) float32 pairs: a grid over 0, 1, the texel centres and the texel boundaries of both axes with the float32 neighbours on both
    sides of each, and 300 seeded random points in [-0.25, 1.25]^2"""
    def axis(n):
        base = np.array([0.0, 1.0] + [(k + 0.5) / n for k in range(n)] + [k / n for k in range(n + 1)], np.float32)
        return np.unique(np.concatenate([base, np.nextafter(base, np.float32(-9)), np.nextafter(base, np.float32(9))]))
    us, vs = axis(w), axis(h)
    grid = [(u, v) for u in us for v in vs]
    assert all(clear_of_weight_steps(u, v, w, h) for u, v in grid)
    rng = np.random.default_rng([seed, h, w])
    rand = []
    while len(rand) < 300:
        u, v = rng.uniform(-0.25, 1.25, 2).astype(np.float32)
        if clear_of_weight_steps(u, v, w, h):
            rand.append((u, v))
    return grid + rand


@pytest.mark.parametrize("shape", sc.FILM_SHAPES, ids=lambda s: "%dx%d" % s)
def test_fetch_equals_float64_rule_at_unlike_shapes(shape):
    """hjo_lut_fetch on the generated tables of tests/shading_cases.py (1 x 1, one row, one column, odd sides both ways, 2 x 64)
    against bilinear_f64 with texel = byte / 255.

    Tolerance, from the float32 expression: the weights are multiples of 2^-16 in [0, 1] and exact; a tap is byte * (1.0f / 255.0f), two
    roundings (the constant and the product); the four weight * tap products round once each, and as the weights sum to 1 their errors
    sum to at most one rounding of the largest tap; three additions of partial sums that never exceed the largest tap.  That is
    2 + 1 + 3 = 6 roundings of 2^-24 relative to the largest tap of the fetch."""
    h, w = shape
    t = sc.film_table(h, w)
    for u, v in fetch_points(h, w, 21):
        want, tmax = bilinear_f64(t, 1.0 / 255.0, u, v)
        got = fetch(t, float(u), float(v)).astype(np.float64)
        assert np.abs(got - want).max() <= 6 * 2.0 ** -24 * tmax, (shape, float(u), float(v), got, want)
