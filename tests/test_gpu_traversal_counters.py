"""Box tests and triangle tests per ray depend on the tree and the ray, not on the shape of the traversal loop or the kernel family.

tests/golden/traversal_counters.json holds the counters of counting launches (HJR_FLAG_STATS) of the bundled Cornell box at 32 x 24, 16 spp,
recorded from the library of commit 6864a79 (the file names it), the last one before the traversal kernels' set-up code was folded: every
layout the options reach (the memory layouts with `short_stack` 2, so that the overflow path runs), both kernel families, all three
integrators; the ten counters `samples` ... `nan_samples` of hjr_stats and `stack_overflow_pushes`.  The 24 launches gave two distinct sets
of the ten counters, one per tree — the BVH2 of the three BVH2 layouts, the BVH4 — whichever family ran, and one overflow count per memory
layout: the file stores each once, and the test asserts every launch against its tree's set, which is also the assertion that the megakernel
and the wavefront kernel count alike.  A change of the loops that tests one box or one triangle more or fewer for any ray shows here.

To record the launches of another build of the library:  HJR_LIB=<path of that libhenjou_hip.so> python tests/test_gpu_traversal_counters.py"""
import json
import os

import pytest

from scene_util import Cornell, hjr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traversal_counters.json")
W, H, SPP = 32, 24, 16
COUNTERS = ("samples", "closest_rays", "shadow_rays", "box_tests_closest", "tri_tests_closest", "box_tests_shadow", "tri_tests_shadow",
            "shaded_hits", "light_samples", "nan_samples")
# name -> (layout options, hjr_stats.lds_mode, tree)
LAYOUTS = {
    "lds": ({}, 1, "bvh2"),
    "lds_stack16": (dict(lds_stack16=1), 2, "bvh2"),
    "bvh2_mem_short2": (dict(lds_bvh=0, bvh_width=2, short_stack=2), 3, "bvh2"),
    "bvh4_mem_short2": (dict(bvh_width=4, short_stack=2), 0, "bvh4"),
}
INTEGRATORS = {"nee": hjr.INTEGRATOR_NEE, "pt": hjr.INTEGRATOR_PT, "mis": hjr.INTEGRATOR_MIS}


@pytest.fixture(scope="module")
def cornell():
    return Cornell()


def count(cornell, layout, pipeline):
    """{integrator: (the ten counters, overflow pushes)} of one device under the layout's options and the kernel family"""
    options, mode, _ = LAYOUTS[layout]
    d = cornell.device(dict(options, pipeline=pipeline))
    try:
        out = {}
        for name, integ in INTEGRATORS.items():
            d.render(cornell.hjr_params(W, H, SPP, integrator=integ, flags=hjr.FLAG_STATS), want_aovs=False)
            st = d.stats()
            assert st["lds_mode"] == mode and st["pipeline"] == pipeline - 1, (layout, pipeline, name, st["lds_mode"], st["pipeline"])
            out[name] = ({k: int(st[k]) for k in COUNTERS}, int(st["stack_overflow_pushes"]))
        return out
    finally:
        d.close()


@pytest.mark.parametrize("pipeline", [1, 2])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_counters_are_the_recorded_ones(cornell, layout, pipeline):
    golden = json.load(open(GOLDEN))
    got = count(cornell, layout, pipeline)
    for name in INTEGRATORS:
        counters, over = got[name]
        print(layout, pipeline, name, counters, over)
        assert counters["samples"] == W * H * SPP
        if "short2" in layout:
            assert over > 0, "the overflow branch never ran"
        assert counters == golden["counters"][LAYOUTS[layout][2]][name], (layout, pipeline, name)
        assert over == golden["stack_overflow_pushes"][layout][name], (layout, pipeline, name)


if __name__ == "__main__":
    c = Cornell()
    for layout in LAYOUTS:
        for pipeline in (1, 2):
            print(layout, pipeline, json.dumps(count(c, layout, pipeline), sort_keys=True))
    print("counted with", hjr.LIB_PATH)
