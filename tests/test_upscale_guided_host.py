"""Host-only parts of the guided 2x upscale (hjr_upscale_guided, option "upscale_guided"; csrc/hjr_denoise.hip.h): the
native checker the GPU kernel is compared with (tests/native/upscale_guided_ref.cpp) against a numpy restatement of the plain bilinear
upscale, its behaviour at silhouettes of synthetic plane G-buffers and on hostile records, the "upscale_guided" key of the render option,
the argument checks that come before any use of the context, and the condition function of tools/upscale_guided_rehearsal.py on a small
oracle frame.  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from scene_util import ROOT, Cornell, hjr
from temporal_util import MISS, plane_gbuffer, wall_camera
from test_device_bvh import _option_json
from upscale_guided_util import all_miss, bilinear_np, bits, changed_pixels, hostile_gbuffer, quality_conditions, upscale_guided_ref

sys.path.insert(0, os.path.join(ROOT, "tools"))
import upscale_guided_rehearsal  # noqa: E402

f32 = np.float32
SHAPES = [(1, 1, 2, 2), (1, 1, 3, 3), (5, 3, 11, 7), (33, 5, 66, 10), (33, 5, 67, 11)]  # iw, ih, ow, oh
NEAR, FAR = np.array([0.25, 0.5, 1.0, 1.0], f32), np.array([2.0, 0.125, 0.75, 0.5], f32)


def _colour(h, w, seed):
    return np.random.default_rng(seed).exponential(0.5, (h, w, 4)).astype(f32)


def two_planes(iw, ih, ow, oh, same_instance):
    """A near rectangle (z = -2, left of x = 0.13) in front of a far wall (z = -5) from one camera at both sizes.  With `same_instance` only
    the plane test can tell them apart (3 units of depth against a pixel footprint of a few hundredths)."""
    cam = wall_camera()
    planes = [(-5.0, 2, 11, -100.0, 100.0), (-2.0, 2 if same_instance else 1, 7, -100.0, 0.13)]
    return cam, plane_gbuffer(iw, ih, cam, planes), plane_gbuffer(ow, oh, cam, planes)


def plane_and_misses(iw, ih, ow, oh):
    cam = wall_camera()
    planes = [(-3.0, 1, 5, -100.0, -0.21)]
    return cam, plane_gbuffer(iw, ih, cam, planes), plane_gbuffer(ow, oh, cam, planes)


@pytest.mark.parametrize("iw,ih,ow,oh", SHAPES)
def test_checker_equals_numpy_bilinear_where_all_or_no_tap_is_valid(iw, ih, ow, oh):
    """Bit-equal wherever the count is 4 or 0, on every kind of record; where it is 1..3 the image may differ, and nowhere else."""
    col = _colour(ih, iw, 3)
    want = bilinear_np(col, ow, oh)
    cam = wall_camera()
    cases = {"all-miss": (all_miss(ih, iw), all_miss(oh, ow)), "hostile": (hostile_gbuffer(ih, iw, 1), hostile_gbuffer(oh, ow, 2)),
             "planes": two_planes(iw, ih, ow, oh, True)[1:], "plane and misses": plane_and_misses(iw, ih, ow, oh)[1:],
             "hits against all-miss": (two_planes(iw, ih, ow, oh, True)[1], all_miss(oh, ow))}
    for name, (lo, hi) in cases.items():
        got, count = upscale_guided_ref(col, lo, cam, hi)
        assert got.shape == (oh, ow, 4) and count.shape == (oh, ow) and count.min() >= 0 and count.max() <= 4, name
        plain = (count == 4) | (count == 0)
        assert np.array_equal(bits(got)[plain], bits(want)[plain]), name
        assert not changed_pixels(got, want)[plain].any() and (changed_pixels(got, want) <= ~plain).all(), name
        if name == "all-miss":
            assert (count == 4).all()
        if name == "hits against all-miss" and iw > 1:
            assert (count == 0).any()


@pytest.mark.parametrize("same_instance", [True, False], ids=["plane test", "instance test"])
def test_no_colour_crosses_between_two_planes(same_instance):
    """Constant colours per side (dyadic, so every weighted sum and the division are exact): each output pixel holds exactly the colour of
    the side its own centre ray hits, where the bilinear upscale mixes the two along the whole edge."""
    iw, ih, ow, oh = 33, 5, 67, 11
    cam, lo, hi = two_planes(iw, ih, ow, oh, same_instance)
    near_lo, near_hi = lo["prim"] == 7, hi["prim"] == 7
    assert near_lo.any() and (~near_lo).any() and near_hi.any() and (~near_hi).any()
    col = np.where(near_lo[..., None], NEAR, FAR).astype(f32)
    got, count = upscale_guided_ref(col, lo, cam, hi)
    assert count.min() >= 1 and ((count > 0) & (count < 4)).any()
    want = np.where(near_hi[..., None], NEAR, FAR).astype(f32)
    assert np.array_equal(bits(got), bits(want))
    mixed = changed_pixels(bilinear_np(col, ow, oh), want)
    assert mixed.any() and np.array_equal(mixed, (count > 0) & (count < 4)), "exactly the pixels with an invalid tap were ramps"


def test_no_colour_crosses_between_a_plane_and_the_background():
    iw, ih, ow, oh = 33, 5, 66, 10
    cam, lo, hi = plane_and_misses(iw, ih, ow, oh)
    hit_lo, hit_hi = lo["prim"] != MISS, hi["prim"] != MISS
    assert hit_lo.any() and (~hit_lo).any()
    col = np.where(hit_lo[..., None], NEAR, FAR).astype(f32)
    got, count = upscale_guided_ref(col, lo, cam, hi)
    assert count.min() >= 1
    assert np.array_equal(bits(got), bits(np.where(hit_hi[..., None], NEAR, FAR).astype(f32)))


def _one_tap(G, T):
    """1 x 1 -> 2 x 2: all four taps of every output pixel are the one low-resolution record, so the count is 4 (valid) or 0."""
    lo = np.zeros((1, 1), hjr.GBUFFER_DTYPE)
    hi = np.zeros((2, 2), hjr.GBUFFER_DTYPE)
    lo[0, 0] = T
    hi[:, :] = G
    got, count = upscale_guided_ref(_colour(1, 1, 9), lo, wall_camera(), hi)
    assert np.isfinite(got).all() and (count == count[0, 0]).all() and count[0, 0] in (0, 4)
    return count[0, 0] == 4


def _rec(prim=5, inst=1, pos=(0.5, 0.25, -3.0), ng=(0.0, 0.0, 2.0)):
    r = np.zeros((), hjr.GBUFFER_DTYPE)
    r["prim"], r["inst"], r["pos"], r["ng"] = prim, inst, np.array(pos, f32), np.array(ng, f32)
    return r


def test_hostile_records_give_invalid_taps_and_no_fault():
    """NaN fails every comparison, an infinite position fails the plane test; prim is compared with the miss value only and inst with inst,
    so arbitrary words are harmless.  (By the rule an infinite normal PARALLEL to the pixel's passes, inf >= inf: such a tap is averaged,
    not indexed with.)  The checker never indexes with a record's field, so nothing here can fault."""
    nan, inf = np.nan, np.inf
    assert _one_tap(_rec(), _rec())
    assert _one_tap(_rec(prim=0xfffffffe), _rec(prim=0x80000000)), "prim words other than the miss value are not compared"
    assert _one_tap(_rec(inst=0xdeadbeef), _rec(inst=0xdeadbeef)) and not _one_tap(_rec(inst=0xdeadbeef), _rec(inst=0xdeadbeee))
    assert _one_tap(_rec(prim=MISS, inst=9, pos=(nan,) * 3), _rec(prim=MISS, ng=(inf,) * 3)), "two misses: nothing else is read"
    assert not _one_tap(_rec(prim=MISS), _rec()) and not _one_tap(_rec(), _rec(prim=MISS))
    for bad in ((nan, 0.25, -3.0), (0.5, 0.25, nan), (0.5, 0.25, inf), (0.5, 0.25, -inf), (inf, -inf, 0.0)):
        assert not _one_tap(_rec(), _rec(pos=bad)), bad
        if np.isnan(bad).any():  # (an infinite position of the PIXEL's record makes its own footprint infinite: inf <= inf passes, by the rule)
            assert not _one_tap(_rec(pos=bad), _rec()), bad
    for bad in ((nan, 0.0, 2.0), (0.0, 0.0, nan), (inf, -inf, 2.0), (0.0, 0.0, -inf), (0.0, 0.0, 0.0), (0.0, 0.0, -2.0), (2.0, 0.0, 0.0)):
        assert not _one_tap(_rec(ng=(1.0, 1.0, 2.0)), _rec(ng=bad)), bad
    for bad in ((nan, 0.0, 2.0), (0.0, 0.0, 0.0), (inf, -inf, 0.0)):
        assert not _one_tap(_rec(ng=bad), _rec()), bad
    # a 1-pixel-high image: fh = 2, the footprint at the point (|view| = 3.05) is 3.05 units
    assert _one_tap(_rec(), _rec(pos=(0.5, 0.25, -5.5))) and not _one_tap(_rec(), _rec(pos=(0.5, 0.25, -6.5))), "2.5 units off the plane pass, 3.5 do not"
    assert _one_tap(_rec(), _rec(pos=(0.9, -0.4, -3.0))), "anywhere on the plane"
    assert _one_tap(_rec(), _rec(ng=(0.0, 0.9, 2.0))) and not _one_tap(_rec(), _rec(ng=(0.0, 1.0, 2.0))), "cos 0.912 passes, cos 0.894 does not"
    # whole images of hostile records at every shape: the checker returns, and only partially valid pixels differ from the bilinear image
    for iw, ih, ow, oh in SHAPES:
        col = _colour(ih, iw, 4)
        got, count = upscale_guided_ref(col, hostile_gbuffer(ih, iw, 11), wall_camera(), hostile_gbuffer(oh, ow, 12))
        assert (changed_pixels(got, bilinear_np(col, ow, oh)) <= ((count > 0) & (count < 4))).all()
    _, count = upscale_guided_ref(_colour(5, 33, 4), hostile_gbuffer(5, 33, 11), wall_camera(), hostile_gbuffer(11, 67, 12))
    assert (count == 0).any() and ((count > 0) & (count < 4)).any(), "the hostile images do exercise both branches"


def test_render_option_parses_upscale_guided(tmp_path):
    """"Henjou_HIP": {"upscale_guided": true} is bit 11 of hjr_render_option.device_bvh_opt: off by default, next to the other keys of the
    field, the struct does not grow for it, and a value that is not a boolean (or 0 / 1) is a parse error."""
    load = lambda extra: hjr.load_render_option(_option_json(tmp_path, extra))  # noqa: E731
    for extra in (None, {}, {"seed": 3}, {"upscale_guided": False}, {"upscale_guided": 0}, {"denoise_variance": True}):
        assert load(extra).device_bvh_opt == 0
    for extra in ({"upscale_guided": True}, {"upscale_guided": 1}):
        o = load(extra)
        assert o.device_bvh_opt == 0x800 and o.denoise_variance == 0
    o = load({"upscale_guided": True, "denoise_variance_spatial": True, "denoise_temporal": True, "firefly_clamp": 8, "device_bvh": True, "device_bvh_opt": 2,
              "device_bvh_instances": True, "device_bvh_graft": True})
    assert o.denoise_variance == 2 and o.device_bvh_opt & 0xff == 2 and o.device_bvh_opt & 0xf00 == 0xf00 and (o.device_bvh_opt >> 16) & 0x7f == 8
    for bad in ("yes", 2, -1, 0.5, [True], {"on": True}, None):
        with pytest.raises(hjr.HjrError, match="upscale_guided"):
            load({"upscale_guided": bad})
    assert hjr.RenderOption.denoise_variance.offset + 4 == C.sizeof(hjr.RenderOption), "nothing was appended"


def test_argument_checks_that_need_no_context():
    """A null context (and with it every other argument check) is HJR_ERR_ARG in both forms before the context is touched."""
    L = hjr.lib()
    col = np.zeros((2, 2, 4), f32)
    lo, hi = all_miss(2, 2), all_miss(4, 4)
    out = np.zeros((4, 4, 4), f32)
    cam = hjr.make_params(2, 2, 1, wall_camera()).camera
    assert L.hjr_upscale_guided(None, 2, 2, col.ctypes.data, lo.ctypes.data, C.byref(cam), hi.ctypes.data, out.ctypes.data, 4, 4) == -1
    assert b"hjr_upscale_guided" in L.hjr_last_error()
    assert L.hjr_upscale_guided_device(None, 2, 2, col.ctypes.data, lo.ctypes.data, C.byref(cam), hi.ctypes.data, out.ctypes.data, 4, 4, None) == -1
    assert L.hjr_upscale_guided(None, 0, 0, None, None, None, None, None, 0, 0) == -1


def test_rehearsal_table_and_condition_function_on_a_small_oracle_frame():
    """tools/upscale_guided_rehearsal.py at 24 x 16 output (12 x 8 x 16 spp, reference 64 spp): the table is complete and finite, silhouette
    pixels do change from both cameras, and the condition function says of the table what an independent evaluation says.  Whether the
    condition HOLDS is a matter of the full-size rehearsal (it does not from x = 3.5), not of this size."""
    table = upscale_guided_rehearsal.rehearse(Cornell(), 24, 16, 16, 64)
    assert list(table) == ["x = 3.5", "scene camera"]
    for name, r in table.items():
        assert r["changed_in_mask"] > 0 and 0 < r["changed_share"] <= r["partial_share"] < 1, name
        assert all(np.isfinite(r[k]) and r[k] > 0 for k in ("e_guided_changed", "e_bilinear_changed", "e_guided_mask", "e_bilinear_mask")), name
    conds = quality_conditions(table)
    assert len(conds) == 1
    print("%s: %s" % (conds[0][0], "holds" if conds[0][1] else "FAILS"))
    assert conds[0][1] == (table["x = 3.5"]["e_guided_changed"] < table["x = 3.5"]["e_bilinear_changed"])
    assert [h for _, h in quality_conditions({"x = 3.5": dict(table["x = 3.5"], e_guided_changed=0.1, e_bilinear_changed=0.1)})] == [False], "equal is not below"
