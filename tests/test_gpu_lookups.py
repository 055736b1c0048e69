"""The thin-film table fetch and the equirect sky fetch on the kernels and through the state that tests/test_gpu_shading_branches.py
does not reach: the memory layouts, 16-bit LDS stacks and the device-built tree, tables that change size on one context, frames split
into work items, sample passes and packed shards, and the textured kernel variant fetching the table.

One scene throughout: shading_cases.film_under_sky, thin-film strips under an open sky with a 5 x 3 table and a 3 x 7 sky bound (unlike
sides both ways, so a swapped size or a wrong stride changes texels), 32 x 24 pixels; tests/test_shading_branches_host.py proves on the
CPU that its frames wrap in u and v of the table and across the azimuth seam of the sky.

Bar: BIT-EXACT float32 equality of the colour, albedo and normal AOVs with the oracle's PORTABLE mode.  The layout and the kernel family
in use are asserted from hjr_stats, never assumed.  No fast-math kernel (not bit-exact by contract)."""
import numpy as np
import pytest

import oracle_binding as ob
import shading_cases as sc
import table_util as tu
from scene_util import device_options, hjr
from test_gpu_parity import assert_bitexact
from test_gpu_progressive import assert_same, one_shot, passes

pytestmark = pytest.mark.gpu

PIPELINES = ("mega", "wf")
COUNTERS = ("samples", "closest_rays", "shadow_rays", "shaded_hits", "light_samples", "nan_samples")
# options -> the lds_modes hjr_stats may report (include/henjou_hip.h: 0 BVH4 from memory, 1 / 2 BVH2 in LDS with 32- / 16-bit stack
# entries, 3 BVH2 from memory)
LAYOUTS = {
    "default": ({}, (1, 2)),
    "stack16": ({"lds_stack16": 1}, (2,)),
    "memory": ({"lds_bvh": 0}, (0,)),
    "memory_bvh2": ({"lds_bvh": 0, "bvh_width": 2}, (3,)),
    "device_bvh": ({"device_bvh": 1}, (0,)),
}
_oracle = {}


def base(**kw):
    c = sc.cases()["film_under_sky"]
    return c.variant(**kw) if kw else c


def key_of(a):
    return None if a is None else (a.shape, a.tobytes())


def oracle_frame(c, iname):
    """(colour, albedo, normal, stats) of the case on the default oracle, computed once per scene, tables, sample count and integrator and
    left unchanged"""
    k = (id(c.arrays), key_of(c.lut_rgba()), key_of(c.sky_rgba), c.spp, iname)
    if k not in _oracle:
        osc = ob.OracleScene(c.oracle_arrays(), ob.MATH_PORTABLE)
        out = osc.render(c.oracle_params(sc.INTEGRATORS[iname]))
        osc.close()
        assert out[3]["nan_samples"] == 0
        for a in out[:3]:
            a.setflags(write=False)
        _oracle[k] = out
    return _oracle[k]


def check_frame(d, c, iname, pipeline, modes, what, **kw):
    """one launch with all AOVs against the oracle frame of `c`; returns hjr_stats"""
    oc, oa, on, _ = oracle_frame(c, iname)
    color, albedo, normal = d.render(c.hjr_params(sc.INTEGRATORS[iname], **kw))
    st = d.stats()
    what = "%s %s %s" % (what, iname, pipeline)
    assert st["pipeline"] == {"mega": 0, "wf": 1}[pipeline], (what, st["pipeline"])
    assert st["lds_mode"] in modes, (what, st["lds_mode"], modes)
    assert_bitexact(color, oc, "aov_color, " + what)
    assert_bitexact(albedo, oa, "aov_albedo, " + what)
    assert_bitexact(normal, on, "aov_normal, " + what)
    return st


# ------------------------------------------------------------------ every layout of both kernel families
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_layouts(pipeline, layout):
    """NEE and MIS on both families, Pathtrace on the megakernel, in the LDS layout the builder picks, with 16-bit LDS stack entries, on
    BVH4 and BVH2 read from memory and on the device-built tree."""
    opts, modes = LAYOUTS[layout]
    c = base()
    with device_options(pipeline=pipeline, **opts):
        d = c.device()
        try:
            for iname in ("nee", "mis") + (("pt",) if pipeline == "mega" else ()):
                check_frame(d, c, iname, pipeline, modes, layout)
        finally:
            d.close()


# ------------------------------------------------------------------ tables that change size on one context
FILM_SEQUENCE = [(5, 3), (2, 64), (1, 1), None, (5, 3)]   # more bytes (the buffer grows), fewer, unbound, bound again
SKY_SEQUENCE = [(7, 3), (32, 64), (1, 1), None, (7, 3)]   # None: the constant sky colour


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_table_changes_on_one_context(pipeline):
    """hjr_set_lut / hjr_set_sky with tables of other sizes, with none, and with the first one again, on a context that keeps its scene:
    each frame is the oracle's frame with that table (a stale width, height or buffer would show)."""
    c0 = base()
    with device_options(pipeline=pipeline):
        d = c0.device()
        try:
            for k, shape in enumerate(FILM_SEQUENCE):
                lut = None if shape is None else sc.film_table(*shape)
                d.set_lut(lut)
                for iname in ("nee", "mis"):
                    check_frame(d, c0.variant(lut=False if lut is None else lut), iname, pipeline, (1, 2), "table %d %s" % (k, shape))
            for k, shape in enumerate(SKY_SEQUENCE):
                sky = None if shape is None else sc.sky_table(*shape)
                d.set_sky(sky)
                for iname in ("nee", "mis"):
                    check_frame(d, c0.variant(sky_rgba=sky), iname, pipeline, (1, 2), "sky %d %s" % (k, shape))
        finally:
            d.close()


# ------------------------------------------------------------------ work splitting
@pytest.mark.parametrize("item_chunks", [1, 2, 4])
def test_item_chunks(item_chunks):
    """32 spp (four chunks) as work items of 1, 2 and 4 chunks of a pixel on the megakernel: NEE and Pathtrace group them, MIS always
    runs single chunks (include/henjou_hip.h, option "item_chunks")"""
    c = base(spp=32)
    d = c.device({"pipeline": 1, "item_chunks": item_chunks})
    try:
        for iname in ("nee", "pt", "mis"):
            st = check_frame(d, c, iname, "mega", (1, 2), "item_chunks %d" % item_chunks)
            assert st["item_chunks"] == (1 if iname == "mis" else item_chunks), (iname, st["item_chunks"])
    finally:
        d.close()


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_sample_passes(pipeline):
    """16 spp in the passes [0, 8) [8, 16): the second pass gives the one-shot frame, which is the oracle's"""
    c = base(spp=16)
    shape = (c.h, c.w, 4)
    with device_options(pipeline=pipeline):
        d = c.device()
        try:
            for iname in ("nee", "mis"):
                check_frame(d, c, iname, pipeline, (1, 2), "one shot")
                p = c.hjr_params(sc.INTEGRATORS[iname])
                got = passes(d, p, [(0, 8), (8, 16)], shape)
                assert_same(got[-1], oracle_frame(c, iname)[:3], "two passes %s %s" % (iname, pipeline))
        finally:
            d.close()


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_packed_shards(pipeline):
    """ranks 0 .. 2 of 3 with HJR_FLAG_PACKED: every in-image slot of a rank's [owned tile][64] buffers holds the oracle frame's pixel"""
    c = base()
    with device_options(pipeline=pipeline):
        d = c.device()
        try:
            for iname in ("nee", "mis"):
                frame = oracle_frame(c, iname)[:3]
                for rank in range(3):
                    n = hjr.owned_tiles(c.w, c.h, rank, 3)
                    assert n > 0
                    p = c.hjr_params(sc.INTEGRATORS[iname], rank=rank, world_size=3, flags=hjr.FLAG_PACKED)
                    got = one_shot(d, p, (n, 64, 4))
                    assert d.stats()["pipeline"] == {"mega": 0, "wf": 1}[pipeline]
                    inside = hjr.pack_tiles(np.ones((c.h, c.w, 4), np.float32), rank, 3)[..., 0] == 1.0
                    assert inside.any()
                    for name, g, f in zip(("color", "albedo", "normal"), got, frame):
                        want = hjr.pack_tiles(f, rank, 3)
                        same = g.view(np.uint32)[inside] == want.view(np.uint32)[inside]
                        assert same.all(), "%s %s rank %d, %s: %d values differ" % (iname, pipeline, rank, name, int((~same).sum()))
        finally:
            d.close()


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_counting_launch(pipeline):
    """a FLAG_STATS launch gives the same bits and the oracle's counters"""
    c = base()
    with device_options(pipeline=pipeline):
        d = c.device()
        try:
            for iname in ("nee", "mis"):
                check_frame(d, c, iname, pipeline, (1, 2), "counting launch", flags=hjr.FLAG_STATS)
                cst, ost = d.stats(), oracle_frame(c, iname)[3]
                for key in COUNTERS:
                    assert cst[key] == ost[key], (iname, pipeline, key, cst[key], ost[key])
        finally:
            d.close()


# ------------------------------------------------------------------ thin film over a base-colour texture
_textured = None


def textured_film():
    """table_util's textured floor with is_thinfilm set on every material that has a base-colour texture: the thickness is then factor x
    texel, and it is the textured kernel variant that fetches the table"""
    global _textured
    if _textured is None:
        s = tu.texture_scene()
        mats = s.arrays["materials"]
        mats["is_thinfilm"] = (mats["basecolor_tex"] >= 0).astype(np.int32)
        assert 0 < mats["is_thinfilm"].sum() < len(mats)
        _textured = s
    return _textured


@pytest.mark.parametrize("layout", ["default", "memory"])
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_thin_film_over_a_texture(pipeline, layout):
    s = textured_film()
    lut = sc.film_table(5, 3)
    w, h, spp = 32, 24, 4
    opts, modes = LAYOUTS[layout]
    with device_options(pipeline=pipeline, **opts):
        d = s.device()
        try:
            d.set_lut(lut)
            for iname in ("nee", "mis"):
                k = ("textured", iname)
                if k not in _oracle:
                    _oracle[k] = ob.OracleScene(dict(s.arrays, lut_rgba=lut), ob.MATH_PORTABLE).render(
                        s.oracle_params(w, h, spp, integrator=sc.INTEGRATORS[iname]))
                    assert _oracle[k][3]["nan_samples"] == 0
                    plain = ob.OracleScene(s.arrays, ob.MATH_PORTABLE).render(s.oracle_params(w, h, spp, integrator=sc.INTEGRATORS[iname]))
                    assert (plain[0] != _oracle[k][0]).any(axis=-1).mean() > 0.05, "the table does not show in the frame"
                oc, oa, on, _ = _oracle[k]
                color, albedo, normal = d.render(s.hjr_params(w, h, spp, integrator=sc.INTEGRATORS[iname]))
                st = d.stats()
                what = "textured film %s %s %s" % (layout, iname, pipeline)
                assert st["pipeline"] == {"mega": 0, "wf": 1}[pipeline] and st["lds_mode"] in modes, (what, st["pipeline"], st["lds_mode"])
                assert_bitexact(color, oc, "aov_color, " + what)
                assert_bitexact(albedo, oa, "aov_albedo, " + what)
                assert_bitexact(normal, on, "aov_normal, " + what)
        finally:
            d.close()
