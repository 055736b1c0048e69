"""The firefly clamp without a GPU (option "firefly_clamp"; include/henjou_hip.h "Firefly clamp", DESIGN.md §4 rule 9): properties of the
numpy float32 restatement (tests/firefly_util.py) on synthetic chunk sums, the "firefly_clamp" key of the render option, the option and
stats mirrors, and the file-level refusals, which come before any device call."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from firefly_util import EPS, f32, firefly_rule, granule_of, lower_median, plain_sum
from scene_util import hjr

ERR_ARG = -1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def synthetic(n, px, seed, spike=None):
    """[n, px, 3] positive chunk sums of about 8 samples each; spike = (chunk, pixel, factor) multiplies one chunk of one pixel."""
    rng = np.random.default_rng(seed)
    c = (rng.random((n, px, 3), dtype=np.float32) * f32(4) + f32(2)).astype(f32)
    if spike:
        k, p, f = spike
        c[k, p] = c[k, p] * f32(f)
    return c


def test_granule_matches_the_library():
    for spp in list(range(1, 70)) + [100, 256, 511, 512, 513, 1024, 1025, 5000]:
        assert granule_of(spp) == hjr.sample_granule(spp), spp


@pytest.mark.parametrize("spp, kappa", [(24, 4), (8 * 3 + 5, 4), (64, 0), (100, 0)])
def test_rule_does_not_act(spp, kappa):
    """m < 4 (24 spp: m = 3; 29 spp: m = 3 and a partial chunk) or kappa = 0: the plain sum's bits and a count of 0, fireflies or not."""
    g = 8
    n = (spp + g - 1) // g
    c = synthetic(n, 11, spp, spike=(1, 3, 1000.0))
    rgb, count, touched = firefly_rule(c, g, spp, kappa)
    assert count == 0 and not touched.any()
    assert np.array_equal(bits(rgb), bits(plain_sum(c) * (f32(1) / f32(spp))))


def test_single_chunk_frame_does_not_act():
    """At most 8 spp the granule is spp itself: one chunk, m = 1."""
    assert granule_of(8) == 8 and granule_of(5) == 5
    c = synthetic(1, 7, 5)
    rgb, count, _ = firefly_rule(c, granule_of(5), 5, 64)
    assert count == 0 and np.array_equal(bits(rgb), bits(c[0] * (f32(1) / f32(5))))


def test_pixels_below_their_limit_keep_the_plain_bits():
    """kappa = 4 on chunk sums within a factor 3 of each other: nothing exceeds 4 x median, every pixel has the plain frame's bits; one
    spiked chunk changes that pixel alone and counts 1."""
    c = synthetic(8, 33, 1)
    plain = plain_sum(c) * (f32(1) / f32(64))
    rgb, count, touched = firefly_rule(c, 8, 64, 4)
    assert count == 0 and not touched.any() and np.array_equal(bits(rgb), bits(plain))
    c2 = synthetic(8, 33, 1, spike=(5, 20, 50.0))
    rgb2, count2, touched2 = firefly_rule(c2, 8, 64, 4)
    assert count2 == 1 and touched2.sum() == 1 and touched2[20]
    others = ~touched2
    assert np.array_equal(bits(rgb2)[others], bits(plain)[others])
    # the scaled chunk weighs exactly its limit: y' = lim up to the rounding of three scaled channels
    y = (c2[..., 0] + c2[..., 1]) + c2[..., 2]
    lim = f32(4) * lower_median(y[:, 20]) + EPS * f32(8)
    s = lim / y[5, 20]
    want = np.zeros(3, f32)
    for k in range(8):
        want = want + (c2[k, 20] * s if k == 5 else c2[k, 20])
    assert np.array_equal(bits(rgb2[20]), bits(want * (f32(1) / f32(64))))
    assert (rgb2[20] < plain_sum(c2)[20] * (f32(1) / f32(64))).all()


@pytest.mark.parametrize("m", [4, 5, 6, 7, 63, 64])
def test_lower_median_even_and_odd(m):
    """Rank (m - 1) // 2 in ascending order: for even m the LOWER of the two middle values; ties and order of arrival do not matter."""
    rng = np.random.default_rng(m)
    v = rng.permutation(m).astype(f32)  # the values 0 .. m-1 in some order
    assert lower_median(v[:, None])[0] == f32((m - 1) // 2)
    tied = np.array([3, 1, 1, 3, 1, 3, 3, 1][:4] * (m // 4 + 1), f32)[:m]
    assert lower_median(tied[:, None])[0] == np.sort(tied)[(m - 1) // 2]
    # the rule uses it: y = 3 * value, one channel each
    c = np.repeat(v[:, None, None], 3, axis=2).astype(f32)
    rgb, count, _ = firefly_rule(c, 8, 8 * m, 1)
    lim = f32(1) * (f32((m - 1) // 2) * f32(3)) + EPS * f32(8)
    assert count == int((v * f32(3) > lim).sum())


def test_partial_chunk_scaling():
    """100 spp: m = 12 full chunks and a partial one of r = 4 samples, whose limit is lim * (4 / 8).  A partial chunk between lim_r and
    lim is scaled (a full chunk of that size would not be), is not among the median's values, and one below lim_r is left alone."""
    g, spp, m, r = 8, 100, 12, 4
    c = np.full((m + 1, 3, 3), f32(1.0))  # y = 3 for every full chunk: med = 3, lim = 12.008, lim_r = 6.004
    c[m, 0] = f32(1.0)   # y = 3  < lim_r
    c[m, 1] = f32(3.0)   # y = 9  > lim_r, < lim
    c[m, 2] = f32(100.0) # far above both
    rgb, count, touched = firefly_rule(c, g, spp, 4)
    lim = f32(4) * f32(3) + EPS * f32(g)
    lim_r = lim * (f32(r) / f32(g))
    assert list(touched) == [False, True, True] and count == 2
    inv = f32(1) / f32(spp)
    full = np.zeros(3, f32)
    for k in range(m):
        full = full + c[k, 0]
    assert np.array_equal(bits(rgb[0]), bits((full + c[m, 0]) * inv))
    for px in (1, 2):
        y = (c[m, px, 0] + c[m, px, 1]) + c[m, px, 2]
        assert np.array_equal(bits(rgb[px]), bits((full + c[m, px] * (lim_r / y)) * inv))
    # the partial chunk does not move the median: a huge one leaves the full chunks' limit where it was
    c2 = c.copy()
    c2[3, 2] = f32(4.5)  # y = 13.5 > lim = 12.008
    assert firefly_rule(c2, g, spp, 4)[1] == 3


def test_all_zero_pixel_stays_zero():
    """A black pixel: med = 0, lim = eps * g > 0, no y exceeds it: +0.0f in every channel and nothing counted; next to a bright pixel."""
    c = np.zeros((8, 2, 3), f32)
    c[:, 1] = f32(2.0)
    rgb, count, touched = firefly_rule(c, 8, 64, 2)
    assert count == 0 and not touched.any()
    assert np.array_equal(bits(rgb[0]), np.zeros(3, np.uint32))
    # a pixel whose median chunk is black and that has ONE lit chunk loses it down to eps * g: the rule's known bias
    c[2, 0] = f32(5.0)
    rgb, count, touched = firefly_rule(c, 8, 64, 2)
    assert count == 1 and touched[0]
    assert abs(float(rgb[0].sum()) - float(EPS * f32(8)) / 64.0) < 1e-9


def _option_json(tmp_path, section, **top):
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    if section is not None:
        ro["Henjou_HIP"] = section
    for k, v in top.items():
        ro[k].update(v)
    path = tmp_path / "render_option.json"
    path.write_text(json.dumps(ro))
    return str(path)


def test_render_option_reads_the_key(tmp_path):
    """"Henjou_HIP": {"firefly_clamp": N} lands in bits 16..22 of hjr_render_option.device_bvh_opt; the BVH bits below stay what they were,
    the struct keeps its size, absent = 0."""
    load = lambda s: hjr.load_render_option(_option_json(tmp_path, s))
    assert load(None).device_bvh_opt == 0 and load({}).device_bvh_opt == 0 and load({"firefly_clamp": 0}).device_bvh_opt == 0
    assert load({"firefly_clamp": 4}).device_bvh_opt == 4 << 16
    assert load({"firefly_clamp": 64}).device_bvh_opt >> 16 == 64
    o = load({"firefly_clamp": 8, "device_bvh": True, "device_bvh_opt": 2, "device_bvh_instances": True, "device_bvh_graft": True})
    assert o.device_bvh_opt & 0xff == 2 and o.device_bvh_opt & 0x300 == 0x300 and (o.device_bvh_opt >> 16) & 0x7f == 8
    for bad in (-1, 65, 2.5, "4", True):
        with pytest.raises(hjr.HjrError, match="firefly_clamp"):
            load({"firefly_clamp": bad})
    assert hjr.RenderOption.denoise_variance.offset + 4 == C.sizeof(hjr.RenderOption)  # nothing was appended


def test_stats_mirror_grew_by_the_counter():
    assert C.sizeof(hjr.StatsV5) == C.sizeof(hjr.StatsV4) + 8 and hjr.StatsV5.firefly_clamped.offset == C.sizeof(hjr.StatsV4)
    assert hjr.StatsV5().struct_size == C.sizeof(hjr.StatsV5)
    assert hjr.StatsV5().as_dict()["firefly_clamped"] == 0


@pytest.mark.parametrize("section, word", [({"firefly_clamp": 4, "passes": 2}, "passes"), ({"firefly_clamp": 4, "noise_threshold": 0.05}, "noise_threshold"),
                                           ({"firefly_clamp": 1, "passes": 64, "noise_threshold": 0.5}, "passes")])
def test_render_file_refuses_the_key_with_sample_passes(tmp_path, section, word):
    """hjr_render_file: "firefly_clamp" with "passes" > 1 or "noise_threshold" > 0 is HJR_ERR_ARG naming both keys, before the scene is
    loaded (the glTF named here does not exist) and before any device call (this test runs without a GPU)."""
    path = _option_json(tmp_path, section, GLTF_file={"gltf_filename": "no_such_scene.gltf"})
    rc = hjr.lib().hjr_render_file(os.fsencode(path), 0)
    err = hjr.lib().hjr_last_error().decode()
    assert rc == ERR_ARG, (rc, err)
    assert "firefly_clamp" in err and word in err and "no_such_scene" not in err
    # "passes": 1 is a whole-frame render: not refused for the key (it goes on to the scene, which is missing)
    path = _option_json(tmp_path, {"firefly_clamp": 4, "passes": 1}, GLTF_file={"gltf_filename": "no_such_scene.gltf"})
    rc = hjr.lib().hjr_render_file(os.fsencode(path), 0)
    assert rc != 0 and "firefly_clamp" not in hjr.lib().hjr_last_error().decode()
