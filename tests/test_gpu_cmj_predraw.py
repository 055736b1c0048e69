"""The first two draws of a BSDF sample are made ahead of the material branch (hjr_kernel.hip.h: bounce_post_trace), by all shading lanes of
the wave together; glass takes the first one only, the multiple-scattering walk takes them as its first step's and draws its later ones
itself.  Which value a sampler takes, and where it leaves the stream, must be what they were: every frame bit-exact against the oracle
(PORTABLE math), all three AOVs.

Frame sizes (render_option_c2.json, which has Disney, metallic and glass surfaces): 4 x 4 x 16 spp — one wave with 16 working lanes;
8 x 8 x 16 spp — one full tile and two chunks; 72 x 40 x 24 spp — several waves, a chunk of 8 that is the item's last, refills in
mid-flight, the hold-back of metallic hits (walks of several lanes together) and the launch tail.
"""
import pytest

import oracle_binding as ob
from scene_util import Cornell, hjr, load_lut
from test_gpu_parity import assert_bitexact

pytestmark = pytest.mark.gpu

SIZES = [(4, 4, 16), (8, 8, 16), (72, 40, 24)]


class Bench:
    """One scene: its oracle and one device per layout, made when first asked for; oracle frames are rendered once."""

    def __init__(self, config):
        self.scene = Cornell(config)
        self.arrays = dict(self.scene.arrays)
        self.lut = load_lut() if config == "render_option_c3.json" else None
        if self.lut is not None:
            self.arrays["lut_rgba"] = self.lut
        self.oracle = ob.OracleScene(self.arrays, ob.MATH_PORTABLE)
        self.devices, self.frames = {}, {}

    def device(self, lds_bvh):
        if lds_bvh not in self.devices:
            d = self.scene.device({"lds_bvh": lds_bvh})
            if self.lut is not None:
                d.set_lut(self.lut)
            self.devices[lds_bvh] = d
        return self.devices[lds_bvh]

    def expected(self, w, h, spp, integrator):
        key = (w, h, spp, integrator)
        if key not in self.frames:
            self.frames[key] = self.oracle.render(self.scene.oracle_params(w, h, spp, integrator=integrator))[:3]
        return self.frames[key]

    def close(self):
        for d in self.devices.values():
            d.close()


@pytest.fixture(scope="module")
def benches():
    made = {}

    def get(config):
        if config not in made:
            made[config] = Bench(config)
        return made[config]
    yield get
    for b in made.values():
        b.close()


def check(bench, w, h, spp, integrator, lds_bvh):
    got = bench.device(lds_bvh).render(bench.scene.hjr_params(w, h, spp, integrator=integrator))
    for a, o, name in zip(got, bench.expected(w, h, spp, integrator), ("aov_color", "aov_albedo", "aov_normal")):
        assert_bitexact(a, o, name)


@pytest.mark.parametrize("lds_bvh", [1, 0])
@pytest.mark.parametrize("integrator", [hjr.INTEGRATOR_NEE, hjr.INTEGRATOR_PT])
@pytest.mark.parametrize("w,h,spp", SIZES)
def test_megakernel_bitexact(benches, w, h, spp, integrator, lds_bvh):
    """NEE and Pathtrace, LDS layout and (lds_bvh 0) the 256-thread memory kernels."""
    check(benches("render_option_c2.json"), w, h, spp, integrator, lds_bvh)


@pytest.mark.parametrize("config", ["render_option_c3.json", "render_option_c4.json"])
def test_thinfilm_and_glass_bitexact(benches, config):
    """Thin-film LUT (c3: the megakernel reads the table's size where it fetches) and negative-index glass (c4: the sample takes the first draw only)."""
    check(benches(config), 8, 8, 16, hjr.INTEGRATOR_NEE, 1)
    check(benches(config), 72, 40, 24, hjr.INTEGRATOR_NEE, 1)


def test_mis_bitexact(benches):
    """MIS runs the wavefront kernels, whose batches hold one material class: the samplers draw for themselves there (the restructured walk)."""
    check(benches("render_option_c2.json"), 8, 8, 16, hjr.INTEGRATOR_MIS, 1)
    check(benches("render_option_c2.json"), 72, 40, 24, hjr.INTEGRATOR_MIS, 1)
