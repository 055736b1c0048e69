"""HJR_FLAG_FAST_MATH beyond the bundled Cornell box: the approximate-arithmetic kernels (a second compilation of the whole shading layer,
hjr_launch_fast_{nee,pt}.hip) on the rare-branch cases of tests/shading_cases.py, on light and material tables past one staging trip, on
material textures, normal maps and equirect skies (the VAR = 2 kernels), on items of several chunks (the SINGLE = false kernels), in
every megakernel layout.

Bar: the comparison rule of tests/fast_math_util.py against the oracle's MATH_LIBM frame at the same sample stream, for
colour, albedo and normal: at most max(2, ceil(0.5 % of the pixels)) + 4 * n_ref pixels off by more than 1e-3 of the pixel's scale, every
value finite, colour alpha 1.  A fast launch has no counting variant and its sample guard zeroes a non-finite sample without a trace, so
an arithmetic fault in a rare branch only darkens pixels: the rule is per pixel for that reason.  tests/test_fast_math_cases_host.py pins
on the CPU that the reference alone stays far inside the cap.  Frames of different kernel instantiations are not compared bit for bit
(contraction is the compiler's choice per instantiation); launches of one kernel are.  Every frame is at most 72 x 48."""
import numpy as np
import pytest

import fast_math_util as fm
import shading_cases as sc
import table_util as tu
from scene_util import device_options, hjr
from test_gpu_parity import assert_bitexact

pytestmark = pytest.mark.gpu

FAST = hjr.FLAG_FAST_MATH
W, H, SPP = fm.TABLE_W, fm.TABLE_H, fm.TABLE_SPP
# options -> the lds_modes hjr_stats may report (include/henjou_hip.h: 0 BVH4 from memory, 1 / 2 BVH2 in LDS with 32- / 16-bit stack
# entries, 3 BVH2 from memory)
LAYOUTS = {
    "default": ({}, (1, 2)),
    "stack16": ({"lds_stack16": 1}, (2,)),
    "memory": ({"lds_bvh": 0}, (0,)),
    "memory_bvh2": ({"lds_bvh": 0, "bvh_width": 2}, (3,)),
}


def fast_frames(d, p, what, want_aovs=True, lds_modes=None, item_chunks=None):
    """one fast-math launch: {aov: frame}; the stats say that the approximate megakernel ran (and in which layout, with which items)"""
    color, albedo, normal = d.render(p, want_aovs=want_aovs)
    st = d.stats()
    assert st["fast_math"] == 1 and st["pipeline"] == 0, (what, st["fast_math"], st["pipeline"])
    if lds_modes is not None:
        assert st["lds_mode"] in lds_modes, (what, st["lds_mode"], lds_modes)
    if item_chunks is not None:
        assert st["item_chunks"] == item_chunks, (what, st["item_chunks"])
    return {"color": color, "albedo": albedo, "normal": normal}


# ------------------------------------------------------------------ a. rare branches, c. lookups at unlike shapes
def test_the_lookup_cases_are_in_the_list():
    names = list(sc.cases())
    assert len(names) == 32
    assert sum(n.startswith("film_") for n in names) == len(sc.FILM_SHAPES) + 1 and "film_under_sky" in names
    assert sum(n.startswith("sky_") for n in names) == len(sc.SKY_CASES)


@pytest.mark.parametrize("iname", list(fm.INTEGRATORS))
@pytest.mark.parametrize("name", list(sc.cases()))
def test_shading_case(name, iname):
    """Every case of tests/shading_cases.py (the walk's exits, p_pow's special arguments, negative-index glass, Disney directions below
    the surface, grazing wo, NaN normals, thin-film tables and skies of unlike shapes at their wrap edges) at its own size."""
    c = sc.cases()[name]
    ref = fm.case_reference(name, iname)
    what = "%s %s" % (name, iname)
    d = c.device()
    try:
        got = fast_frames(d, c.hjr_params(fm.INTEGRATORS[iname], flags=FAST), what)
    finally:
        d.close()
    ref.check(got, what)


def test_mis_ignores_the_flag():
    c = sc.cases()["film_under_sky"]
    d = c.device()
    try:
        flagged = d.render(c.hjr_params(hjr.INTEGRATOR_MIS, flags=FAST))
        assert d.stats()["fast_math"] == 0
        exact = d.render(c.hjr_params(hjr.INTEGRATOR_MIS))
    finally:
        d.close()
    for aov, a, b in zip(fm.AOVS, flagged, exact):
        assert_bitexact(a, b, "MIS with the flag against MIS without, " + aov)


# ------------------------------------------------------------------ b. tables and textures
def table_frames(name, iname, what, lds_modes):
    s = tu.scene(name)
    ref = fm.table_reference(name, iname)
    d = s.device()
    try:
        p = s.hjr_params(W, H, SPP, integrator=fm.INTEGRATORS[iname], flags=FAST)
        full = fast_frames(d, p, what, lds_modes=lds_modes)
        lean = fast_frames(d, p, what + " colour only", want_aovs=False, lds_modes=lds_modes)
    finally:
        d.close()
    ref.check(full, what)
    ref.check(lean, what + " colour only")


@pytest.mark.parametrize("iname", list(fm.INTEGRATORS))
@pytest.mark.parametrize("name", [n for n in fm.TABLE_SCENES if n != "textured"])
def test_tables(name, iname):
    """171 and 200 light rows, 205 and 210 material rows (the staging loops of the LDS layout take a second trip) and the texture scene
    without its metallic-roughness slot, with the AOVs and colour only."""
    table_frames(name, iname, "%s %s" % (name, iname), (1, 2))


@pytest.mark.parametrize("iname", list(fm.INTEGRATORS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_textured_every_layout(layout, iname):
    """All four texture slots and the normal map (the VAR = 2 kernels) in every megakernel layout, with the AOVs and colour only."""
    opts, modes = LAYOUTS[layout]
    with device_options(**opts):
        table_frames("textured", iname, "textured %s %s" % (layout, iname), modes)


# ------------------------------------------------------------------ d. items of several chunks
@pytest.mark.parametrize("iname", list(fm.INTEGRATORS))
@pytest.mark.parametrize("item_chunks", [2, 4])
def test_item_chunks(item_chunks, iname):
    """The SINGLE = false kernels: the bundled scene at the ragged 21 x 13 and 32 spp (4 chunks of 8), items of 2 and of 4 chunks."""
    s = fm.cornell()
    ref = fm.chunk_reference(iname)
    what = "item_chunks %d %s" % (item_chunks, iname)
    d = s.device({"item_chunks": item_chunks})
    try:
        p = s.hjr_params(fm.CHUNK_W, fm.CHUNK_H, fm.CHUNK_SPP, integrator=fm.INTEGRATORS[iname], flags=FAST)
        full = fast_frames(d, p, what, item_chunks=item_chunks)
        lean = fast_frames(d, p, what + " colour only", want_aovs=False, item_chunks=item_chunks)
    finally:
        d.close()
    ref.check(full, what)
    ref.check(lean, what + " colour only")


@pytest.mark.parametrize("iname", list(fm.INTEGRATORS))
def test_item_chunks_textured(iname):
    """VAR = 2 and SINGLE = false at once: the textured scene at 16 spp as items of two chunks."""
    s = tu.scene("textured")
    ref = fm.table_reference("textured", iname, fm.TEX_CHUNK_SPP)
    what = "textured item_chunks 2 %s" % iname
    d = s.device({"item_chunks": 2})
    try:
        got = fast_frames(d, s.hjr_params(W, H, fm.TEX_CHUNK_SPP, integrator=fm.INTEGRATORS[iname], flags=FAST), what, item_chunks=2)
    finally:
        d.close()
    ref.check(got, what)


# ------------------------------------------------------------------ e. same kernel, same bits
def test_same_kernel_same_bits():
    """On one device and the textured scene: a repeated fast frame, three tile shards assembled and a frame in two sample passes equal the
    one-shot fast frame bit for bit."""
    s = tu.scene("textured")
    spp, R = fm.TEX_CHUNK_SPP, 3
    d = s.device()
    try:
        def render(**kw):
            frames = d.render(s.hjr_params(W, H, spp, flags=FAST, **kw))
            assert d.stats()["fast_math"] == 1
            return frames

        first = render()
        again = render()
        shards = [render(rank=r, world_size=R) for r in range(R)]
        for b, e in ((0, 8), (8, spp)):
            passes = render(sample_begin=b, sample_end=e)
        after = render()
    finally:
        d.close()
    fm.table_reference("textured", "nee", spp).check(dict(zip(fm.AOVS, first)), "textured one-shot at %d spp" % spp)
    for i, aov in enumerate(fm.AOVS):
        assert_bitexact(again[i], first[i], "repeated fast frame, " + aov)
        assert_bitexact(after[i], first[i], "fast frame after shards and passes, " + aov)
        acc = np.zeros_like(first[i])
        for r in range(R):
            mask = hjr.owned_tile_mask(W, H, r, R)
            assert np.all(shards[r][i][~mask] == 0)
            assert_bitexact(shards[r][i][mask][None], first[i][mask][None], "shard %d of %d, %s" % (r, R, aov))
            acc += shards[r][i]
        assert_bitexact(acc, first[i], "sum of the shards, " + aov)
        assert_bitexact(passes[i], first[i], "last of two sample passes, " + aov)
