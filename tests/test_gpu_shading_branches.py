"""Shading-branch parity: the small scenes of tests/shading_cases.py, each built to drive named rare branches of the shading layer (the
multiple-scattering GGX walk's exits, the negative-index glass, Disney sampling below the surface, p_pow's special returns, the light
index clamp, the zero-contribution test of NEE / MIS), on both kernel families against the default oracle.
tests/test_shading_branches_host.py proves on the CPU that the frames take those branches.

Bar: BIT-EXACT float32 equality of the colour, albedo and normal AOVs with the oracle's PORTABLE mode; with FLAG_STATS the ray, hit,
light-sample and NaN counters are the oracle's and every NaN sample the GPU locates is one of the oracle's.  The fast-math kernels (not
bit-exact by contract) render the same cases in tests/test_gpu_fast_math_cases.py, under a per-pixel rule.  No full-size frame: every
parameter set is one frame of at most 32 x 32 pixels."""
import pytest

import oracle_binding as ob
import shading_cases as sc
from scene_util import device_options, hjr
from test_gpu_parity import assert_bitexact

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "closest_rays", "shadow_rays", "shaded_hits", "light_samples", "nan_samples")
_oracle = {}


def oracle_frame(name, iname):
    """(OracleScene, colour, albedo, normal, stats) of one case and integrator on the default oracle, computed once"""
    if (name, iname) not in _oracle:
        c = sc.cases()[name]
        if name not in _oracle:
            _oracle[name] = ob.OracleScene(c.oracle_arrays(), ob.MATH_PORTABLE)
        _oracle[name, iname] = (_oracle[name],) + _oracle[name].render(c.oracle_params(sc.INTEGRATORS[iname]))
    return _oracle[name, iname]


@pytest.mark.parametrize("pipeline", ("mega", "wf"))
@pytest.mark.parametrize("iname", list(sc.INTEGRATORS))
@pytest.mark.parametrize("name", list(sc.cases()))
def test_shading_case(name, iname, pipeline):
    c = sc.cases()[name]
    integ = sc.INTEGRATORS[iname]
    osc, oc, oa, on, ost = oracle_frame(name, iname)
    what = "%s %s %s" % (name, iname, pipeline)
    with device_options(pipeline=pipeline):
        d = c.device()
        try:
            color, albedo, normal = d.render(c.hjr_params(integ))
            st = d.stats()
            counted, _, _ = d.render(c.hjr_params(integ, flags=hjr.FLAG_STATS), want_aovs=False)
            cst = d.stats()
        finally:
            d.close()
    assert st["pipeline"] == {"mega": 0, "wf": 1}[pipeline], (what, st["pipeline"])
    assert_bitexact(color, oc, "aov_color, " + what)
    assert_bitexact(albedo, oa, "aov_albedo, " + what)
    assert_bitexact(normal, on, "aov_normal, " + what)
    assert_bitexact(counted, oc, "counting launch, " + what)
    for key in COUNTERS:
        assert cst[key] == ost[key], (what, key, cst[key], ost[key])
    assert len(cst["nan_where"]) == min(ost["nan_samples"], 8), (what, cst["nan_where"])
    op = c.oracle_params(integ)
    for (x, y, s) in cst["nan_where"]:
        assert osc.sample_is_nan(op, x, y, s), "%s: sample %d of pixel (%d, %d) is NaN on the GPU only" % (what, s, x, y)
