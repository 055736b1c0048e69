"""The case list of tests/shading_cases.py reaches the branches it was built for: proved on the CPU with the oracle's named branch
counters (oracle/hjr_oracle.c, HJO_HIT; a build with -DHJO_BRANCH_COUNTERS that tests/oracle_binding.py makes in a temporary
directory).  tests/test_gpu_shading_branches.py then renders the same frames on the GPU against the default oracle, so a GPU error
in one of these branches changes frames that are compared bit for bit.

Every named branch is taken at least MIN_HITS times over the case list, and in at least one frame of every integrator that can reach
it, or it stands in EXEMPT with a written reason.  The counts of a run with 1 thread and of one with 4 threads are equal, and equal
to the recorded tests/golden/shading_branch_counts.json (regenerate with `python tests/test_shading_branches_host.py --record` after
changing a case on purpose)."""
import json
import os
import sys

import numpy as np
import pytest

import oracle_binding as ob
import shading_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shading_branch_counts.json")
MIN_HITS = 8
ALL = ("nee", "pt", "mis")


def reach(name):
    """the integrators that can take the branch"""
    if name.startswith("nee_"):
        return ("nee",)
    if name.startswith("mis_"):
        return ("mis",)
    if name.startswith("light_"):
        return ("nee", "mis")  # Pathtrace samples no light
    if name in ("atan2_y_zero", "atan2_x_zero"):
        # An exactly axis-aligned direction reaches the sky lookup only as the (0, 0, 1) a walk of more than five orders leaves in wi,
        # on a surface whose shading normal lies on an axis.  That exit returns a zero BSDF: NEE and Pathtrace end the path at the
        # next roulette test (throughput 0) without tracing it, MIS traces its BSDF-sampled ray before it looks at the weight.
        return ("mis",)
    return ALL


# kind "unreachable": no render can take the branch; the reason cites what excludes it.
# kind "search": nothing excludes it, no sample of the stated CPU search took it.
RANGE = ("p_pow has two callers.  ms_G1_Height passes the base ms_C1(h) in [0, 1] (fminf / fmaxf clamp, which also turns a NaN into 0) and the "
         "exponent ms_Lambda(wi) >= 0 (wi.y <= 0 returns before).  ms_sampleHeight passes the base 1 - U with U in [0, 1], so 0 or at "
         "least 2^-24, and the exponent 1 / ms_Lambda(wr), which lies in [-1, 0) for a downward wr and is positive for an upward one.  So "
         "t = y * log(x) <= 24 ln 2 = 16.7.  ")
NAN_SEARCH = ("Inside a walk a non-finite hr or wr needs normalize() of an exactly zero vector in a later step (a sampled half vector that "
              "cancels the view direction; a NaN view direction leaves at the first step, see pow_nan_arg); nothing excludes it.  Not found in the case list nor in a search of 6000 further frames (the cases head_on_mirror, "
              "grazing_lens, rough_metal_pit, shading_normals and glass with the seeds 100 .. 499 under NEE, Pathtrace and MIS: "
              "3.6e7 samples).  ")
EXEMPT = {
    "lambda_up_exit": ("unreachable", "ms_Lambda is called by ms_G1_Height after its own `wi.y > 0.9999f` return and by ms_sampleHeight after its "
                       "`wr.y > 0.9999f` return: v.y > 0.9999 never arrives."),
    "lambda_down_exit": ("unreachable", "ms_G1_Height returns at `wi.y <= 0.0f` before it calls ms_Lambda, ms_sampleHeight returns at "
                         "`wr.y < -0.9999f` before it does: v.y < -0.9999 never arrives."),
    "g1_up_exit": ("unreachable", "ms_G1_Height's only caller is ms_sampleHeight, after its `wr.y > 0.9999f` return."),
    "msggx_wi_below": ("unreachable", "ms_sample sets wi only where the walk escapes, and ms_sampleHeight returns FLT_MAX only for wr.y > 0.9999 or "
                       "for U > 1 - G1 with G1 = 0 for wr.y <= 0 (ms_G1_Height), which no U <= 1 satisfies: an escaping wr points up.  The "
                       "other exits leave wi = (0, 0, 1) or the caller's (0, 1, 0).  `wi.y < 0` is dead; `order > 5` is the live half."),
    "disney_lobe_clearcoat": ("unreachable", "Listed as dead because clearcoatWeight is the constant 0 in disney_sample (cw == 0).  Strictly it is "
                              "reachable in principle: `select_p < dw + sw` fails for a lobe pick of exactly 1.0, or within an ulp of it "
                              "where dw + sw rounds below 1 (about one draw in 4e7).  No case drives it: the draws of exactly 1.0 that "
                              "tests/golden/find_unit_draws.py found are spent on a metallic floor, where they are height draws."),
    "cosine_sampling": ("unreachable", "no integrator calls it (d_sampleDiffuse restates it); it is exported for the known-answer tests only."),
    "pow_neg_base": ("unreachable", RANGE + "No base is negative."),
    "pow_inf_base": ("unreachable", RANGE + "No base exceeds 1."),
    "pow_denormal_base": ("unreachable", RANGE + "The smallest positive ms_C1 is 0.5 * 2^-24: no base lies in (0, FLT_MIN)."),
    "pow_overflow": ("unreachable", RANGE + "t > 88.7 never arrives."),
    "exp_rescale": ("unreachable", RANGE + "n > 127 needs t > 88.03 (the denoiser's dn_weight, no part of a render, passes e <= 0)."),
    "exp_underflow": ("unreachable", "hjo_p_pow returns 0 at `t < -87.0f` before it calls p_exp, dn_weight clamps to -87, and "
                      "floor(1.442695 * -87 + 0.5) = -126: n < -126 never arrives."),
    "pow_t_nan": ("unreachable", "y == 0, x == 1 (the only x with log(x) == 0) and NaN arguments return earlier in hjo_p_pow, log(x) is finite for "
                  "the finite positive x that remain: y * log(x) is never 0 * inf."),
    "walk_nan_exit": ("search", NAN_SEARCH + "ms_sample's `(hr != hr) || (wr.z != wr.z)`."),
    "pow_nan_arg": ("unreachable", "The bases ms_C1(h) and 1 - U are NaN-free (fminf / fmaxf clamp; U is a draw).  An exponent is NaN only for a "
                    "NaN direction.  At the first step of a walk C1(hr) == 1 and hjo_p_pow returns at `x == 1.0f` before it looks for a NaN; "
                    "the walk then escapes (U > 0) or, for U == 0, meets 1 - U == 1 the same way.  At every later step ms_sample's "
                    "`wr.z != wr.z` exit has returned before ms_sampleHeight sees the NaN wr.  (nan_normal drives exactly this: pow_x_one.)"),
}
# the issue allows the second kind for the light index clamp, the walk's NaN exit and p_pow's t != t and overflow returns only; of
# these only the walk's NaN exit needs it
SEARCH_ALLOWED = {"walk_nan_exit"}


def run_counts(nthreads, frames=None):
    """{case: {integrator: {branch: count}}} of the whole case list on the counting oracle; frames: filled with the colour images"""
    out = {}
    with ob.counting_oracle() as names:
        for name, c in sc.cases().items():
            osc = ob.OracleScene(c.oracle_arrays(), ob.MATH_PORTABLE)
            out[name] = {}
            for iname, integ in sc.INTEGRATORS.items():
                ob.branch_reset()
                color, _, _, _ = osc.render(c.oracle_params(integ), nthreads=nthreads, want_aovs=False)
                out[name][iname] = {k: v for k, v in ob.branch_counts().items() if v}
                if frames is not None:
                    frames[name, iname] = color
            osc.close()
        out["_names"] = list(names)
    return out


@pytest.fixture(scope="module")
def counts():
    frames = {}
    return run_counts(1, frames), frames


def totals(counts):
    names = counts["_names"]
    tot = {n: dict.fromkeys(ALL, 0) for n in names}
    for case, per in counts.items():
        if case == "_names":
            continue
        for iname, c in per.items():
            for k, v in c.items():
                tot[k][iname] += v
    return tot


def test_every_branch_is_counted_or_exempt(counts):
    tot = totals(counts[0])
    short = []
    for name, t in tot.items():
        if name in EXEMPT:
            assert sum(t.values()) == 0, "%s is exempt and taken %s: drop the exemption" % (name, t)
            continue
        if sum(t.values()) < MIN_HITS or any(t[i] == 0 for i in reach(name)):
            short.append((name, t))
    assert not short, "branches the case list does not reach: %s" % short


def test_exemptions_are_of_the_two_kinds(counts):
    names = set(counts[0]["_names"])
    for name, (kind, reason) in EXEMPT.items():
        assert name in names, name
        assert kind in ("unreachable", "search") and len(reason) > 40, name
    assert {n for n, (kind, _) in EXEMPT.items() if kind == "search"} == SEARCH_ALLOWED
    assert all("search of" in EXEMPT[n][1] and "samples" in EXEMPT[n][1] for n in SEARCH_ALLOWED)  # the size of the search is stated


def test_counts_do_not_depend_on_the_thread_count(counts):
    assert run_counts(4) == counts[0]


def test_counts_are_the_recorded_ones(counts):
    """a change of a case (or of the oracle) that loses a branch shows here, per case and integrator"""
    with open(GOLDEN) as f:
        recorded = json.load(f)
    fresh = {k: v for k, v in counts[0].items() if k != "_names"}
    assert sorted(fresh) == sorted(recorded)
    for case in fresh:
        for iname in ALL:
            assert fresh[case][iname] == recorded[case][iname], (case, iname)


def test_counting_build_renders_the_default_builds_frames(counts):
    """the counters change no arithmetic: the frames of the counting build are those of the library oracle/Makefile builds"""
    for name, c in sc.cases().items():
        osc = ob.OracleScene(c.oracle_arrays(), ob.MATH_PORTABLE)
        for iname, integ in sc.INTEGRATORS.items():
            color, _, _, st = osc.render(c.oracle_params(integ), nthreads=4, want_aovs=False)
            assert np.array_equal(color.view(np.uint32), counts[1][name, iname].view(np.uint32)), (name, iname)
            # the zero-normal patch of shading_normals and the NaN-normal patch of nan_normal give non-finite samples in every
            # integrator (more than the 8 the GPU locates), no other case has any
            assert (st["nan_samples"] > 8) if name in ("shading_normals", "nan_normal") else (st["nan_samples"] == 0), (name, iname, st["nan_samples"])
        osc.close()


def test_case_frames_are_small():
    for c in sc.cases().values():
        assert c.w <= 32 and c.h <= 32 and 4 <= c.spp <= 32 and c.arrays["indices"].size // 3 <= 300, c.name


if __name__ == "__main__" and "--record" in sys.argv:
    rec = run_counts(1)
    del rec["_names"]
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", GOLDEN)
