"""Scene tables beyond the few rows every other scene has: many emitter triangles under rotated, non-uniformly scaled and mirrored
instances, hundreds of materials, light lists that are shuffled / hold a triangle twice / miss an emissive triangle, a zero-area emitter,
the LDS budget decision at its boundaries, and material textures in every slot of the material row (tests/table_util.py).

Bar: BIT-EXACT float32 equality of all three AOVs, and of the colour-only launch, with the oracle's PORTABLE mode, which recomputes every
light from light_prim_ids, the instance transform and the raw vertices per sample and never sees the product's per-frame light table.
The staging loops of an LDS-resident layout copy the tables with a 1024-thread workgroup: a light row is 6 float4 and a material row 5,
so the second trip starts at 171 lights and at 205 materials.  The layout in use is asserted from hjr_stats, never assumed.  The inputs
are pinned on the CPU by tests/test_scene_tables_host.py."""
import numpy as np
import pytest

import oracle_binding as ob
import table_util as tu
from scene_util import hjr
from test_gpu_parity import assert_bitexact
from test_gpu_variants import knobs

pytestmark = pytest.mark.gpu

W, H, SPP = 72, 48, 5
NEE, PT, MIS = hjr.INTEGRATOR_NEE, hjr.INTEGRATOR_PT, hjr.INTEGRATOR_MIS
PIPELINES = ("mega", "wf")
COUNTERS = ("samples", "closest_rays", "shadow_rays", "shaded_hits", "light_samples", "nan_samples")
LDS_MODES, MEMORY_MODES = (1, 2), (0, 3)

_oracle_cache = {}


def oracle_frame(name, integrator):
    """(colour, albedo, normal, stats) of the named scene on the oracle, computed once"""
    k = (name, integrator)
    if k not in _oracle_cache:
        s = tu.scene(name)
        _oracle_cache[k] = ob.OracleScene(s.arrays, ob.MATH_PORTABLE).render(s.oracle_params(W, H, SPP, integrator=integrator))
    return _oracle_cache[k]


def check(name, env, pipeline, integrators, layout, scene=None, expect_pipeline=None, nan_ok=False, counters=False):
    """One device with the knobs set: for each integrator all three AOVs and the colour-only launch against the oracle frame of scene
    `name` (`scene`: a variant of it that must render the same frame).  layout: the lds_modes hjr_stats may report.  Returns
    {integrator: stats of the launch with AOVs}."""
    s = scene if scene is not None else tu.scene(name)
    out = {}
    with knobs(HJR_PIPELINE=pipeline, **env):
        d = s.device()
        try:
            for integ in integrators:
                oc, oa, on, ost = oracle_frame(name, integ)
                assert nan_ok or ost["nan_samples"] == 0
                what = "%s %s %s integrator %d" % (name, env, pipeline, integ)
                color, albedo, normal = d.render(s.hjr_params(W, H, SPP, integrator=integ))
                st = out[integ] = d.stats()
                for key in ("pipeline", "lds_mode", "stack_need", "stack_lds_entries"):
                    assert key in st
                assert st["lds_mode"] in layout, (what, st["lds_mode"], layout)
                if expect_pipeline != "any":  # "any": which family runs a request is the library's decision (the budget edges)
                    assert st["pipeline"] == {"mega": 0, "wf": 1}[pipeline], (what, st["pipeline"])
                assert_bitexact(color, oc, "aov_color, " + what)
                assert_bitexact(albedo, oa, "aov_albedo, " + what)
                assert_bitexact(normal, on, "aov_normal, " + what)
                lean, _, _ = d.render(s.hjr_params(W, H, SPP, integrator=integ), want_aovs=False)
                assert_bitexact(lean, oc, "colour-only launch, " + what)
                if counters:
                    counted, _, _ = d.render(s.hjr_params(W, H, SPP, integrator=integ, flags=hjr.FLAG_STATS), want_aovs=False)
                    assert_bitexact(counted, oc, "counting launch, " + what)
                    cst = d.stats()
                    for key in COUNTERS:
                        assert cst[key] == ost[key], (what, key, cst[key], ost[key])
                    st["stack_overflow_pushes"] = cst["stack_overflow_pushes"]
        finally:
            d.close()
    return out


# ------------------------------------------------------------------ light table sizes
@pytest.mark.parametrize("lds", [True, False], ids=["lds", "memory"])
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("name", list(tu.LIGHT_COUNTS))
def test_light_table_sizes(name, pipeline, lds):
    """1, 3, 64, 171 and 200 light rows (171 = the first count whose staging loop takes a second trip) in the layout the builder picks
    — an LDS-resident one for every count, which is asserted — and read from memory; the counters of a counting launch are the oracle's."""
    assert tu.scene(name).arrays["light_prim_ids"].size == tu.LIGHT_COUNTS[name]
    check(name, {} if lds else {"HJR_LDS_BVH": 0}, pipeline, (NEE, PT, MIS), LDS_MODES if lds else MEMORY_MODES, counters=True)


def test_light_table_contents():
    """What can be said about the per-frame light table without restating its arithmetic: one row per list entry, in list order, with the
    list's prim id and the list's emission (the bit-exact frames check the rest)."""
    for name in ("lights64", "shuffled", "duplicate", "odd_emission"):
        s = tu.scene(name)
        d = s.device()
        try:
            rows = d.copy_frame_data(hjr.FRAME_LIGHTS).reshape(-1, 24)
        finally:
            d.close()
        ids = s.arrays["light_prim_ids"]
        assert rows.shape[0] == ids.size
        assert np.array_equal(rows[:, 19].view(np.uint32), ids), name
        assert np.array_equal(rows[:, [7, 11, 15]].view(np.uint32), s.arrays["light_prim_emission"].view(np.uint32)), name


# ------------------------------------------------------------------ light list shapes
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("name", ["shuffled", "duplicate", "unlisted", "odd_emission", "ends", "empty_before"])
def test_light_list_shapes(name, pipeline):
    """A list out of triangle order, a triangle listed twice, an emissive triangle that is not listed (MIS: its pdf is the reference's
    getLightPDF, which does not consult the list), a row whose emission is not the material's, emitters in the first and the last
    instance, an empty instance in front of an emitter instance."""
    check(name, {}, pipeline, (NEE, MIS), LDS_MODES)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_empty_light_list_with_emissive_surfaces(pipeline):
    """is_light materials and no light list: a BSDF-sampled emitter hit under MIS gets the reference's light pdf 1 / (area x 0) = inf
    and the weight 0 (the hit triangle's own area, whatever the list holds)."""
    check("no_list", {}, pipeline, (NEE, PT, MIS), LDS_MODES, counters=True)
    check("no_list", {"HJR_LDS_BVH": 0}, pipeline, (MIS,), MEMORY_MODES)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_zero_area_emitter(pipeline):
    """pdf = inf in one light row: nothing under NEE and Pathtrace, NaN samples under MIS — as many as the oracle has, zeroed alike."""
    st = check("zero_area", {}, pipeline, (NEE, PT, MIS), LDS_MODES, nan_ok=True, counters=True)
    assert oracle_frame("zero_area", MIS)[3]["nan_samples"] > 0 and oracle_frame("zero_area", NEE)[3]["nan_samples"] == 0
    assert st[MIS]["lds_mode"] in LDS_MODES


# ------------------------------------------------------------------ material table sizes
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("name", list(tu.MATERIAL_COUNTS))
def test_material_table_sizes(name, pipeline):
    """2, 65, 205 and 210 materials (205 = the first count whose staging loop takes a second trip), every one of them referenced; the
    emissive materials are the last rows."""
    assert tu.scene(name).arrays["materials"].size == tu.MATERIAL_COUNTS[name]
    check(name, {}, pipeline, (NEE, MIS), LDS_MODES)


def test_material_table_from_memory():
    check("mats205", {"HJR_LDS_BVH": 0}, "mega", (NEE,), MEMORY_MODES)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_both_tables_past_one_staging_trip(pipeline):
    """200 lights and 210 materials, LDS-resident with 32-bit stack entries"""
    st = check("both", {}, pipeline, (NEE, MIS), (1,))
    assert st[NEE]["stack_need"] >= 10


# ------------------------------------------------------------------ the device builder keeps the host's light table
@pytest.mark.parametrize("opt", [0, 2])
def test_device_builder(opt):
    env = {"HJR_DEVICE_BVH": 1}
    if opt:
        env["HJR_DEVICE_BVH_OPT"] = opt
    check("lights64", env, "mega", (NEE, MIS), MEMORY_MODES)
    check("lights64", env, "wf", (NEE, MIS), MEMORY_MODES)


# ------------------------------------------------------------------ LDS budget edges
def test_wavefront_lds_scene_with_short_stacks():
    """LDSBVH + SPILL of the wavefront kernel directly: the scene in LDS, two stack entries per lane, the rest overflows to memory"""
    st = check("lights64", {"HJR_SHORT_STACK": 2}, "wf", (NEE, MIS), LDS_MODES, counters=True)
    for integ in (NEE, MIS):
        assert st[integ]["stack_lds_entries"] == 2 < st[integ]["stack_need"], st[integ]
        assert st[integ]["stack_overflow_pushes"] > 0, "the overflow branch never ran"


PAD_MAX = 2048  # 2048 x 80 B = 160 KiB of materials alone: the whole LDS of a CU, so no LDS-resident layout can hold this scene


def test_lds_budget_edges():
    """The 200-light / 210-material scene with more and more unreferenced materials behind its table: each costs 80 B of the LDS budget
    and changes no pixel.  The padding counts at which the builder's layout changes are found by bisection on hjr_stats.lds_mode (the
    budget formulas are not restated here); on both sides of every change both kernel families render the oracle's frame.  Among these
    launches are the wavefront kernel with an LDS-resident scene whose stacks no longer fit (LDSBVH + SPILL) and its refusal of a
    scene that leaves fewer than four stack entries per lane (falls back to the megakernel)."""
    base = tu.scene("both")
    modes = {}

    def mode_at(k):
        if k not in modes:
            s = base.with_padding(k)
            d = s.device()
            try:
                d.render(s.hjr_params(8, 8, 1), want_aovs=False)  # hjr_stats reports the layout of the last launch
                modes[k] = d.stats()["lds_mode"]
            finally:
                d.close()
        return modes[k]

    def last_of(mode, lo, hi):
        """largest k in [lo, hi) with mode_at(k) == mode, given mode_at(lo) == mode != mode_at(hi) and one change in between"""
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if mode_at(mid) == mode:
                lo = mid
            else:
                hi = mid
        return lo

    assert mode_at(0) == 1, "the base scene must start in the 32-bit LDS layout"
    assert mode_at(PAD_MAX) == 0, "a material table as large as the LDS cannot be LDS-resident"
    # the first padding count that leaves mode 1 for good; what follows it is mode 2 (16-bit stack entries still fit) or 0
    k1 = last_of(1, 0, PAD_MAX)
    points = [k1, k1 + 1]
    if mode_at(k1 + 1) == 2:
        k2 = last_of(2, k1 + 1, PAD_MAX)
        points += [k2, k2 + 1]
        assert mode_at(k2 + 1) == 0
    else:
        assert mode_at(k1 + 1) == 0
    assert all(modes[a] == modes[b] or a in points for a, b in zip(sorted(modes), sorted(modes)[1:])), sorted(modes.items())  # one change per boundary
    print("lds budget edges: padding %s -> lds_mode %s" % (points, [mode_at(k) for k in points]))
    spill, fallback = [], []
    for k in points:
        s = base.with_padding(k)
        layout = (mode_at(k),)
        st = check("both", {}, "mega", (NEE, MIS), layout, scene=s)
        st = check("both", {}, "wf", (NEE, MIS), layout, scene=s, expect_pipeline="any")
        for integ in (NEE, MIS):
            assert st[integ]["stack_need"] > 0
            if st[integ]["pipeline"] == 1 and st[integ]["lds_mode"] in LDS_MODES and st[integ]["stack_lds_entries"] < st[integ]["stack_need"]:
                spill.append((k, integ))
            if st[integ]["pipeline"] == 0:
                fallback.append((k, integ))
        print("  padding %d: lds_mode %d, wavefront request ran as pipeline %d with %d of %d stack entries in LDS"
              % (k, mode_at(k), st[NEE]["pipeline"], st[NEE]["stack_lds_entries"], st[NEE]["stack_need"]))
    assert spill, "no wavefront launch with an LDS-resident scene and spilling stacks among the probed points"
    assert fallback, "no wavefront request fell back to the megakernel among the probed points"


# ------------------------------------------------------------------ texture slots of the material row
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_material_texture_slots(pipeline):
    """Metallic-roughness alone, with a base colour, with base colour and normal map, one image in two slots; four images of unlike
    shapes (1x1, 3x5, 64x2, 17x17; sRGB and linear), so that every descriptor offset differs; uv from -1.5 to 2.5."""
    check("textured", {}, pipeline, (NEE, MIS), LDS_MODES)
    check("textured_no_mr", {}, pipeline, (NEE, MIS), LDS_MODES)
    for integ in (NEE, MIS):
        a, b = oracle_frame("textured", integ)[0], oracle_frame("textured_no_mr", integ)[0]
        assert (a != b).any(axis=-1).mean() > 0.01, "the metallic-roughness slot does not show in the frame"


def test_material_texture_slots_from_memory():
    check("textured", {"HJR_LDS_BVH": 0}, "mega", (NEE, MIS), MEMORY_MODES)
