"""Small scenes built to drive the guarded special cases of the shading layer (the multiple-scattering GGX walk, the negative-index
glass, Disney sampling, p_pow's special returns, the light pick, the zero-contribution test of NEE / MIS).  A handful of triangles
each, assembled in numpy in the style of tests/table_util.py; frames of at most 32 x 32 at 4 to 32 spp.
The film_* and sky_* cases bind generated thin-film tables and equirect skies of unlike, odd, one-row and one-column shapes and look
where the lookups wrap (the counters lut_* / sky_* of the oracle).
tests/test_shading_branches_host.py proves on the CPU, with the oracle's named branch counters, which branch each case takes;
tests/test_gpu_shading_branches.py renders the same frames on the GPU against the default oracle."""
import numpy as np

import oracle_binding as ob
import table_util as tu
from scene_util import hjr, new_device

F32 = np.float32
UP = (0.0, 1.0, 0.0)


_lut = None


def load_lut():
    """the bundled thin-film LUT as uint8 [h, w, 4], decoded here so that the CPU proof needs no product library; oracle and device get
    this same array"""
    global _lut
    if _lut is None:
        import os
        from PIL import Image
        _lut = np.ascontiguousarray(Image.open(os.path.join(hjr.ASSETS, "LUT", "Thin_Film_LUT.png")).convert("RGBA"), dtype=np.uint8)
    return _lut


def look_at(pos, target, f, up_hint=UP):
    """camera dict: unit dir / right / up in float32, `f` the focal length in units of half the frame height"""
    pos, target = np.asarray(pos, float), np.asarray(target, float)
    d = target - pos
    d /= np.linalg.norm(d)
    right = np.cross(d, np.asarray(up_hint, float))
    right /= np.linalg.norm(right)
    up = np.cross(right, d)
    return {"pos": [float(F32(x)) for x in pos], "dir": [float(F32(x)) for x in d], "up": [float(F32(x)) for x in up],
            "right": [float(F32(x)) for x in right], "f": float(f)}


def material(basecolor=(0.8, 0.8, 0.8), metallic=0.0, roughness=0.5, ior=1.0, emission=None, glass=False, thinfilm=False, sheen=0.0):
    m = np.zeros((), hjr.MATERIAL_DTYPE)
    m["basecolor"], m["metallic"], m["roughness"], m["ior"], m["sheen"] = basecolor, metallic, roughness, ior, sheen
    m["transmission"] = 1.0 if glass else 0.0
    m["ideal_specular"], m["is_thinfilm"] = int(glass), int(thinfilm)
    if emission is not None:
        m["emission"], m["is_light"] = emission, 1
    for k in tu.TEX_KEYS:
        m[k] = -1
    return m


class Mesh:
    """triangles with per-vertex normals and one material id each"""

    def __init__(self):
        self.v, self.n, self.m = [], [], []

    def tri(self, a, b, c, mat, normals=None):
        a, b, c = (np.asarray(p, float) for p in (a, b, c))
        if normals is None:
            fn = np.cross(b - a, c - a)
            normals = [fn / np.linalg.norm(fn)] * 3
        elif np.ndim(normals) == 1:
            normals = [normals] * 3
        self.v.append([a, b, c]); self.n.append([np.asarray(q, float) for q in normals]); self.m.append(mat)

    def quad(self, a, b, c, d, mat, normals=None):
        """a, b, c, d counter-clockwise seen from the side the face normal points to"""
        self.tri(a, b, c, mat, normals)
        self.tri(a, c, d, mat, normals)

    def floor(self, x0, z0, x1, z1, mat, y=0.0, normals=None):
        """a quad on y = const that faces up"""
        self.quad((x0, y, z0), (x0, y, z1), (x1, y, z1), (x1, y, z0), mat, normals)

    def ceiling(self, x0, z0, x1, z1, mat, y):
        """a quad on y = const that faces down (the emitters)"""
        self.quad((x0, y, z0), (x1, y, z0), (x1, y, z1), (x0, y, z1), mat)

    def box(self, lo, hi, mat):
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        self.floor(x0, z0, x1, z1, mat, y=y1)
        self.ceiling(x0, z0, x1, z1, mat, y=y0)
        self.quad((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0), mat)  # -z
        self.quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1), mat)  # +z
        self.quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0), mat)  # -x
        self.quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1), mat)  # +x

    def wedge(self, x0, x1, z0, z1, h, mat):
        """a prism on y = 0 whose ridge runs along x at z = (z0 + z1) / 2, height h"""
        zm = 0.5 * (z0 + z1)
        self.ceiling(x0, z0, x1, z1, mat, y=0.0)
        self.quad((x0, 0, z0), (x0, h, zm), (x1, h, zm), (x1, 0, z0), mat)
        self.quad((x0, 0, z1), (x1, 0, z1), (x1, h, zm), (x0, h, zm), mat)
        self.tri((x0, 0, z0), (x0, 0, z1), (x0, h, zm), mat)
        self.tri((x1, 0, z0), (x1, h, zm), (x1, 0, z1), mat)

    def arrays(self, mats):
        n = len(self.v)
        mats = np.array(mats, hjr.MATERIAL_DTYPE)
        lights = [i for i in range(n) if mats[self.m[i]]["is_light"]]
        return dict(vertices=np.array(self.v, F32).reshape(-1, 3), normals=np.array(self.n, F32).reshape(-1, 3),
                    texcoords=np.zeros((3 * n, 2), F32), indices=np.arange(3 * n, dtype=np.uint32),
                    material_ids=np.array(self.m, np.uint32), prim_offsets=np.zeros(1, np.uint32),
                    transforms=tu.IDENTITY.reshape(1, 12).copy(), inv_transforms=tu.IDENTITY.reshape(1, 12).copy(), materials=mats,
                    light_prim_ids=np.array(lights, np.uint32),
                    light_prim_emission=np.array([mats[self.m[i]]["emission"] for i in lights], F32).reshape(-1, 3), textures=[])


class Case:
    """One frame: scene arrays, camera, size, sample stream, sky and whether the thin-film LUT / an equirect sky is bound.
    lut: True binds the bundled table, a uint8 [h, w, 4] array binds that table."""

    def __init__(self, name, arrays, camera, w, h, spp, frame=1, seed=1, sky=(0.05, 0.06, 0.08), lut=False, sky_rgba=None, targets="",
                 ibl_intensity=1.0):
        assert w <= 32 and h <= 32 and 4 <= spp <= 32
        self.name, self.arrays, self.camera, self.w, self.h, self.spp = name, arrays, camera, w, h, spp
        self.frame, self.seed, self.sky, self.lut, self.sky_rgba, self.targets = frame, seed, sky, lut, sky_rgba, targets
        self.ibl_intensity = ibl_intensity

    def variant(self, **kw):
        """a copy with the given attributes replaced (the scene arrays are shared)"""
        import copy
        c = copy.copy(self)
        for k, v in kw.items():
            assert hasattr(c, k), k
            setattr(c, k, v)
        assert c.w <= 32 and c.h <= 32 and 4 <= c.spp <= 32
        return c

    def lut_rgba(self):
        """the table oracle and device get, or None"""
        if isinstance(self.lut, np.ndarray):
            return self.lut
        return load_lut() if self.lut else None

    def oracle_arrays(self):
        a = dict(self.arrays)
        if self.lut_rgba() is not None:
            a["lut_rgba"] = self.lut_rgba()
        if self.sky_rgba is not None:
            a["sky_rgba"] = self.sky_rgba
        return a

    def oracle_params(self, integrator):
        return ob.make_params(self.w, self.h, self.spp, self.camera, frame=self.frame, seed=self.seed, integrator=integrator, sky=self.sky,
                              ibl_intensity=self.ibl_intensity)

    def hjr_params(self, integrator, **kw):
        return hjr.make_params(self.w, self.h, self.spp, self.camera, frame=self.frame, seed=self.seed, integrator=integrator,
                               sky=self.sky, ibl_intensity=self.ibl_intensity, **kw)

    def device(self, options=None):
        d = new_device(options)
        try:
            d.upload_arrays(self.arrays)
            d.set_transforms(self.arrays["transforms"], self.arrays["inv_transforms"])
            if self.lut_rgba() is not None:
                d.set_lut(self.lut_rgba())
            if self.sky_rgba is not None:
                d.set_sky(self.sky_rgba)
        except Exception:
            d.close()
            raise
        return d


LIGHT = material(emission=(12.0, 11.0, 10.0))


def head_on_mirror():
    """A roughness-0 metallic plane seen straight down through a long lens: the middle of the frame is within 0.72 degrees of the normal
    (cos > 0.9999: the walk starts with its `< -0.9999` case and leaves through `> 0.9999`), the corners are at 1.01 degrees (the general
    case with alpha clamped to 1e-4, where 1 + a^2 tan^2 rounds to 1, Lambda is 0 and p_pow sees y == 0)."""
    m = Mesh()
    m.floor(-50, -50, 50, 50, 0)
    m.ceiling(-2, -2, 2, 2, 1, y=10.0)
    return Case("head_on_mirror", m.arrays([material((0.9, 0.8, 0.7), metallic=1.0, roughness=0.0), LIGHT]),
                look_at((0, 5, 0), (0, 0, 0), 80.0, up_hint=(0, 0, 1)), 16, 16, 8,
                targets="height_down_start height_up_exit pow_y_zero")


def equirect_sky():
    rng = np.random.default_rng(11)
    sky = np.zeros((8, 16, 4), F32)
    sky[..., :3] = rng.uniform(0.0, 2.0, (8, 16, 3)).astype(F32)
    return sky


def grazing_lens():
    """A plane seen from a hair above it through a lens of focal length 2000: |wo.y| < 5e-4 in every row and < 1e-4 near the horizon.
    Left half rough metal (the walk's grazing return), right half Disney (sampled directions below the surface); the rows above
    the horizon and the far distance miss into an equirect sky (p_atan2 / p_acos of the sky lookup)."""
    m = Mesh()
    m.floor(-2000, 0, 0, 20000, 0)
    m.floor(0, 0, 2000, 20000, 1)
    m.ceiling(-500, 0, 500, 20000, 2, y=300.0)
    mats = [material((0.9, 0.6, 0.3), metallic=1.0, roughness=0.6), material((0.3, 0.6, 0.9), metallic=0.2, roughness=0.4, sheen=0.5), LIGHT]
    return Case("grazing_lens", m.arrays(mats), look_at((0, 0.01, -1), (0, 0.01, 0), 2000.0), 32, 32, 8, sky_rgba=equirect_sky(),
                targets="height_graze disney_wi_below atan2_*")


def rough_metal_pit():
    """A trench of roughness-1 metal (flat floor, one vertical and one sloping wall, open at both ends) under a small light and an
    equirect sky: walks of more than five orders, whose exit leaves wi = (0, 0, 1) and pdf as the caller set it.  Under MIS that
    direction is traced: from the floor it is the world direction (0, 0, -1), from the vertical wall (0, 1, -0), both of which miss
    into the sky lookup with an exactly zero argument of p_atan2."""
    m = Mesh()
    m.floor(-1, -4, 1, 4, 0)
    m.quad((-1, 0, -4), (-1, 3, -4), (-1, 3, 4), (-1, 0, 4), 0)
    m.quad((1, 0, -4), (1, 0, 4), (4, 3, 4), (4, 3, -4), 0)
    m.ceiling(-0.5, -0.5, 0.5, 0.5, 1, y=6.0)
    return Case("rough_metal_pit", m.arrays([material((0.95, 0.9, 0.85), metallic=1.0, roughness=1.0), LIGHT]),
                look_at((0.8, 5, 0.2), (0, 0.5, 0), 2.0, up_hint=(0, 0, 1)), 24, 24, 16, sky_rgba=equirect_sky(),
                targets="walk_order_gt5 msggx_order_gt5 pow_zero_result atan2_y_zero atan2_x_zero")


def glass():
    """A slab (ior 1.5), a wedge (ior 2.4) and a second slab (ior 1.33) of ideal-specular glass over a lit floor, the light in view
    through them: entering, leaving, total internal reflection; under MIS the light pdf of a specular bounce is 0."""
    m = Mesh()
    m.floor(-6, -6, 6, 6, 0)
    m.box((-3.0, 0.5, -1.0), (-1.2, 0.9, 1.0), 1)
    m.wedge(-0.9, 0.9, -1.0, 1.0, 1.2, 2)
    m.box((1.2, 0.5, -1.0), (3.0, 1.4, 1.0), 3)
    m.ceiling(-4, -3, 4, -2, 4, y=4.0)
    m.floor(-4, 2, 4, 3, 4, y=0.02)  # a light strip on the floor, facing up
    mats = [material((0.7, 0.7, 0.7), roughness=0.8), material(glass=True, roughness=0.0, ior=1.5),
            material(glass=True, roughness=0.0, ior=2.4), material(glass=True, roughness=0.0, ior=1.33), LIGHT]
    return Case("glass", m.arrays(mats), look_at((0, 3.5, -5), (0, 0.6, 0), 1.6), 32, 24, 8,
                targets="glass_* refract_tir mis_lightpdf_specular nee_contrib_zero")


def shading_normals():
    """Sixteen floor patches whose vertex normals are not the face's: the six axis directions (n.y = +1 and -1, n.z = +1, -1, -0.0),
    normals that lean far enough for wo.y < 0 (the counters disney_wo_below and walk_wo_below), and one patch of zero-length normals (non-finite samples in every integrator), on a
    Disney and on a metallic material in turn."""
    axes = [(0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), (0, 1, -0.0), (0.6, -0.8, 0.0)]
    lean = [(0.0, -0.3, 0.954), (0.7, 0.1, -0.707), (-0.5, 0.5, 0.707), (0.0, 0.2, -0.98)]
    m = Mesh()
    k = 0
    for j in range(4):
        for i in range(4):
            mat = (i + j) % 2
            if k < 8:
                nn = axes[k]
            elif k == 15:
                nn = (0.0, 0.0, 0.0)  # wo.y == 0 exactly: the BSDF divides by it, the NaN / Inf guard of the sample zeroes the result
            else:
                a, b = np.array(lean[k % 4], float), np.array(lean[(k + 1) % 4], float)
                nn = [a / np.linalg.norm(a), b / np.linalg.norm(b), a / np.linalg.norm(a)]
            m.floor(-4 + 2 * i, -4 + 2 * j, -2 + 2 * i, -2 + 2 * j, mat, normals=nn)
            k += 1
    m.ceiling(-2, -2, 2, 2, 2, y=5.0)
    mats = [material((0.8, 0.5, 0.3), metallic=0.0, roughness=0.3), material((0.9, 0.9, 0.6), metallic=1.0, roughness=0.4), LIGHT]
    return Case("shading_normals", m.arrays(mats), look_at((1.0, 7, -6), (0, 0, 0), 1.4), 32, 32, 4, targets="basis_* disney_wo_below walk_wo_below sample_nan_guard")


def coloured_lights():
    """A blue-only and a green-only emitter over surfaces whose base colour has zero channels, and a glass block: the zero-contribution
    test of NEE / MIS sees (0, 0, z), (0, y, 0) and (0, 0, 0)."""
    m = Mesh()
    m.floor(-4, -4, 0, 4, 0)
    m.floor(0, -4, 4, 4, 1)
    m.box((-0.8, 0.3, -0.8), (0.8, 0.9, 0.8), 2)
    m.ceiling(-3, -1, -1, 1, 3, y=4.0)
    m.ceiling(1, -1, 3, 1, 4, y=4.0)
    mats = [material((1.0, 0.0, 0.0), roughness=0.7), material((0.0, 0.9, 0.0), metallic=1.0, roughness=0.5),
            material(glass=True, roughness=0.0, ior=1.5), material(emission=(0.0, 0.0, 9.0)), material(emission=(0.0, 7.0, 0.0))]
    return Case("coloured_lights", m.arrays(mats), look_at((0, 4.5, -6), (0, 0.3, 0), 1.5), 24, 16, 8, targets="*_contrib_partial *_contrib_zero")


def many_lights():
    """table_util's 200-emitter scene at a small frame (the light pick over a long list)"""
    s = tu.scene("lights200")
    return Case("many_lights", s.arrays, s.camera, 32, 24, 4, sky=tu.SKY, targets="light_pick")


# (seed, depth) of a sample stream that holds a draw of exactly 1.0 in a 32 x 32 frame at 32 spp, frame 1: found by
# tests/golden/find_unit_draws.py, a search over the seeds 1 .. 9000 at depth 2 and 1 .. 3000 at depths 4 and 5 (2.9e8 / 9.8e7 /
# 9.8e7 draws; about one draw in 4e7 is 1.0).  At a first hit on a non-emissive surface depth 2 is the light pick of NEE and MIS (index == n_lights: the
# clamp) and the first height draw of Pathtrace's walk; depth 4 is the first height draw of MIS' walk, depth 5 that of NEE's.  A
# height draw of 1.0 on a downward ray makes p_pow(1 - U, 1 / Lambda) a power of zero with a negative exponent: the height becomes
# -1, and every later step of that walk takes a power of zero with a positive exponent.
UNIT_DRAWS = [(946, 2), (2424, 2), (8427, 2), (8572, 2), (402, 4), (1174, 4), (1054, 5), (2219, 5)]


def unit_draw(seed, depth):
    """A rough metal floor that fills the frame under five emitter triangles, rendered with a seed whose stream holds a draw of
    exactly 1.0 (UNIT_DRAWS)."""
    m = Mesh()
    m.floor(-40, -40, 40, 40, 0)
    for i in range(5):
        m.tri((-4 + 2 * i, 6, 1), (-3 + 2 * i, 6, 1), (-4 + 2 * i, 6, 2 + 0.2 * i), 1 + i)
    mats = [material((0.9, 0.7, 0.5), metallic=1.0, roughness=0.5)] + [material(emission=(3.0 + i, 8.0 - i, 2.0 * i + 1.0)) for i in range(5)]
    return Case("unit_draw_%d" % seed, m.arrays(mats), look_at((0, 4, -4), (0, 0, 0), 3.0), 32, 32, 32, seed=seed,
                targets="light_index_clamp pow_zero_base_*" if depth == 2 else "pow_zero_base_*")


def nan_normal():
    """A roughness-0 mirror floor seen straight down, and over the camera, out of its view, a rough metal patch whose vertex normals
    hold a NaN (bits 0x7fc00000), under an equirect sky.  The mirrored ray meets the patch at depth 1, so the AOVs stay finite; there
    the local view direction is NaN, the walk leaves at its first step (C1 == 1: p_pow returns at x == 1 before it looks for a NaN)
    with a NaN direction, and that ray is traced into the sky lookup: p_atan2 with a NaN argument, a non-finite sample."""
    m = Mesh()
    m.floor(-50, -50, 50, 50, 0)
    m.ceiling(-0.04, -0.04, 0.04, 0.04, 1, y=8.0)
    m.ceiling(-3, 1, 3, 2, 2, y=9.0)
    a = m.arrays([material((0.9, 0.8, 0.7), metallic=1.0, roughness=0.0), material((0.8, 0.8, 0.8), metallic=1.0, roughness=0.4), LIGHT])
    a["normals"][6:12] = np.array([np.nan, 1.0, 0.0], F32)
    return Case("nan_normal", a, look_at((0, 5, 0), (0, 0, 0), 80.0, up_hint=(0, 0, 1)), 16, 16, 4, sky_rgba=equirect_sky(),
                targets="atan2_nan_arg sample_nan_guard")


def thin_film(lut):
    """Thin-film on a metallic-0.51 (msGGX sampling, Disney evaluation) and a metallic-0.5 material side by side"""
    m = Mesh()
    m.floor(-4, -4, 0, 4, 0)
    m.floor(0, -4, 4, 4, 1)
    m.ceiling(-2, -2, 2, 2, 2, y=4.0)
    mats = [material((0.35, 0.6, 0.8), metallic=0.51, roughness=0.3, thinfilm=True),
            material((0.65, 0.6, 0.8), metallic=0.5, roughness=0.3, thinfilm=True), LIGHT]
    return Case("thin_film_lut" if lut else "thin_film_no_lut", m.arrays(mats), look_at((0, 3, -5), (0, 0, 0), 1.5), 24, 16, 4, lut=lut,
                targets="bsdf_is_ggx bsdf_not_ggx lut_bound" if lut else "lut_unbound")


def no_lights():
    """no light list: light_sample's first return"""
    m = Mesh()
    m.floor(-4, -4, 4, 4, 0)
    return Case("no_lights", m.arrays([material((0.6, 0.7, 0.8), roughness=0.6)]), look_at((0, 3, -5), (0, 0, 0), 1.5), 8, 8, 4,
                sky=(0.8, 0.7, 0.6), targets="light_none")


# ------------------------------------------------------------------ thin-film tables and skies of unlike shapes, at their wrap edges
FILM_SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (5, 3), (2, 64)]  # [h, w]
SKY_SHAPES = [(3, 7), (7, 3), (1, 1), (1, 5), (5, 1), (32, 64)]


def _all_differ(a):
    """no two rows and no two columns of [h, w, c] are equal"""
    h, w = a.shape[:2]
    return len({a[j].tobytes() for j in range(h)}) == h and len({a[:, i].tobytes() for i in range(w)}) == w


def film_table(h, w):
    """A generated thin-film table, uint8 [h, w, 4]: seeded random bytes, R, G and B unlike in every texel, no two rows or columns
    equal, so that a wrong stride, a swapped size or a swapped channel changes the values fetched."""
    rng = np.random.default_rng([5, h, w])
    t = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    t[..., 1] = np.where(t[..., 1] == t[..., 0], t[..., 0] ^ 0x55, t[..., 1])
    t[..., 2] = np.where((t[..., 2] == t[..., 0]) | (t[..., 2] == t[..., 1]), t[..., 0] ^ t[..., 1] ^ 0xff, t[..., 2])
    t[..., 3] = 255
    assert _all_differ(t[..., :3]) and (t[..., 0] != t[..., 1]).all() and (t[..., 1] != t[..., 2]).all() and (t[..., 0] != t[..., 2]).all()
    return t


def sky_table(h, w):
    """A generated equirect sky, float32 [h, w, 4]: texels drawn from [0, 3), up to three of them 1e4 (a sun), all finite; channels,
    rows and columns unlike."""
    rng = np.random.default_rng([6, h, w])
    t = np.zeros((h, w, 4), F32)
    t[..., :3] = rng.uniform(0.0, 3.0, (h, w, 3)).astype(F32)
    for k in rng.choice(h * w, min(3, h * w // 4), replace=False):
        t[k // w, k % w, int(rng.integers(0, 3))] = 1e4
    assert np.isfinite(t).all() and _all_differ(t[..., :3])
    return t


# (metallic, roughness) of the eight film strips: Disney (metallic <= 0.5) and, at 0.51, the material the walk samples and Disney evaluates
FILM_STRIPS = [(0.0, 0.3), (0.51, 0.2), (0.3, 0.5), (0.5, 0.3), (0.51, 0.4), (0.2, 0.25), (0.5, 0.6), (0.0, 0.35)]


def film_thickness(w):
    """basecolor.x (the thickness: the table's u coordinate) of the eight strips for a table of w columns: both ends of [0, 1], the first
    and the last texel centre, a hair inside each end, and two inner values"""
    return [F32(x) for x in (0.0, 1.0, 0.5 / w, 1.0 - 0.5 / w, 1e-3, 0.999, 0.37, 0.71)]


def film_mesh(m, mat0=0):
    """eight floor strips of 2 x 16 along z, materials mat0 .. mat0 + 7"""
    for i in range(8):
        m.floor(-8 + 2 * i, -8, -6 + 2 * i, 8, mat0 + i)


def film_lights(m, mat):
    """an emitter over the strips, and a low one across their far end that faces the camera: lit from there a strip seen at a grazing
    angle has its half vector near the normal and the light direction near the plane (cosines near 0: the table's first row)"""
    m.ceiling(-3, -2, 3, 2, mat, y=5.0)
    m.quad((-8, 0.05, 8.2), (-8, 0.8, 8.2), (8, 0.8, 8.2), (8, 0.05, 8.2), mat)


def film_materials(w):
    return [material((t, 0.55 + 0.05 * (i % 3), 0.9 - 0.1 * (i % 4)), metallic=mt, roughness=r, thinfilm=True)
            for i, (t, (mt, r)) in enumerate(zip(film_thickness(w), FILM_STRIPS))]


def film(h, w):
    """Thin-film strips under an emitter, seen from low over the floor so that grazing and near-normal cosines (the table's v coordinate)
    both occur, with a generated table of shape [h, w] bound."""
    m = Mesh()
    film_mesh(m)
    film_lights(m, 8)
    return Case("film_%dx%d" % (h, w), m.arrays(film_materials(w) + [LIGHT]), look_at((0, 1.0, -9), (0, 0, 0), 1.2), 32, 24, 8,
                lut=film_table(h, w), targets="lut_u_* lut_v_*")


def sky_mesh(m, mat0=0):
    """a small diffuse floor with a metallic and a glass patch on it and an emitter over it: materials mat0 .. mat0 + 3"""
    m.floor(-2, -2, 2, 2, mat0)
    m.floor(-1.5, -1.5, -0.2, 1.5, mat0 + 1, y=0.01)
    m.box((0.3, 0.01, -1.2), (1.5, 0.5, 1.2), mat0 + 2)
    m.ceiling(-0.6, -0.6, 0.6, 0.6, mat0 + 3, y=3.0)


SKY_MATERIALS = [material((0.7, 0.6, 0.5), roughness=0.8), material((0.9, 0.85, 0.7), metallic=1.0, roughness=0.25),
                 material(glass=True, roughness=0.0, ior=1.5), LIGHT]
# views of the sky scene: most of each frame is open sky
SKY_VIEWS = {
    "seam": ((4, 1, 0.3), (-4, 1.2, 0), 1.0, UP),            # along -x: the azimuth seam (u = 0 | 1) runs down the frame
    "zenith": ((0.05, 0.1, -1.0), (0.05, 30, -0.9), 0.5, (0, 0, 1)),  # up from the floor, the glass box at one side: the rows at v = 0
    "nadir": ((3.4, 2, 0.2), (3.4, -30, 0.25), 1.0, (0, 0, 1)),   # straight down past the floor's edge: the rows at v = 1
    "nadir_long": ((2.6, 2, 0.2), (2.6, -30, 0.25), 3.0, (0, 0, 1)),  # the same through a longer lens: within 3 degrees of straight down
    "side": ((0.5, 1.5, -6), (0, 0.8, 0), 1.5, UP),
}


def sky(h, w, view):
    """The sky scene under a generated equirect sky of shape [h, w], ibl_intensity 0.75, in one of SKY_VIEWS."""
    m = Mesh()
    sky_mesh(m)
    pos, target, f, up = SKY_VIEWS[view]
    return Case("sky_%dx%d_%s" % (h, w, view), m.arrays(SKY_MATERIALS), look_at(pos, target, f, up_hint=up), 32, 24, 4,
                sky_rgba=sky_table(h, w), ibl_intensity=0.75, targets="sky_u_* sky_v_*")


def film_under_sky():
    """The film strips (5 x 3 table) under an open 3 x 7 sky instead of a dark constant one, seen along -x over the strips so that the
    azimuth seam crosses the frame: both lookups in one frame.  tests/test_gpu_lookups.py renders it on every kernel layout."""
    m = Mesh()
    film_mesh(m)
    film_lights(m, 8)
    return Case("film_under_sky", m.arrays(film_materials(3) + [LIGHT]), look_at((7, 1.2, -7), (-6, 0.3, 0), 1.2), 32, 24, 4,
                lut=film_table(5, 3), sky_rgba=sky_table(3, 7), ibl_intensity=0.75, targets="lut_u_* lut_v_* sky_u_*")


SKY_CASES = [(3, 7, "seam"), (7, 3, "zenith"), (1, 1, "side"), (1, 5, "seam"), (5, 1, "nadir"), (32, 64, "nadir_long")]

_cases = None


def cases():
    """the case list, built once: {name: Case}"""
    global _cases
    if _cases is None:
        lst = [head_on_mirror(), grazing_lens(), rough_metal_pit(), glass(), shading_normals(), coloured_lights(), many_lights(),
               thin_film(True), thin_film(False), no_lights(), nan_normal()] + [unit_draw(*sd) for sd in UNIT_DRAWS]
        lst += [film(h, w) for h, w in FILM_SHAPES] + [sky(*hwv) for hwv in SKY_CASES] + [film_under_sky()]
        _cases = {c.name: c for c in lst}
    return _cases


INTEGRATORS = {"nee": ob.INTEGRATOR_NEE, "pt": ob.INTEGRATOR_PT, "mis": ob.INTEGRATOR_MIS}
