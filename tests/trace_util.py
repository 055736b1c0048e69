"""Scenes, adversarial ray classes and the brute-force ground truth of the ray-level traversal tests (tests/test_trace_rays_host.py pins
them on the CPU, tests/test_gpu_trace.py hands them to hjr_trace_rays).  Everything is generated from fixed seeds; float32 throughout."""
import numpy as np

import oracle_binding as ob
from scene_util import hjr

F32 = np.float32
TMIN = F32(0.001)
NO_PRIM = 0xFFFFFFFF
IDENTITY = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], F32)
OFFSET = (1000.0, -500.0, 250.0)
GRID_Z = F32(0.25)
GRID_FIRST, GRID_COUNT = 512, 512  # prim ids of the quad grid in the soup


# ------------------------------------------------------------------ scenes
def soup_triangles(seed=20251):
    """The hostile soup: [1185, 3, 3] float32 vertices, prim ids in the order of the list below."""
    rng = np.random.default_rng(seed)
    tris = []
    # 512 random small triangles in [-0.9, 0.9]^3, edges <= 0.2
    # (edges of 0.15 .. 0.2 that enclose 35 .. 60 degrees: the third edge is then no longer than the longer of the two)
    v0 = rng.uniform(-0.7, 0.7, (512, 3))
    u1 = rng.normal(size=(512, 3)); u1 /= np.linalg.norm(u1, axis=1, keepdims=True)
    w1 = np.cross(u1, rng.normal(size=(512, 3))); w1 /= np.linalg.norm(w1, axis=1, keepdims=True)
    th = np.radians(rng.uniform(35, 60, (512, 1)))
    e1 = rng.uniform(0.15, 0.2, (512, 1)) * u1
    e2 = rng.uniform(0.15, 0.2, (512, 1)) * (np.cos(th) * u1 + np.sin(th) * w1)
    tris.append(np.stack([v0, v0 + e1, v0 + e2], 1))
    # 16 x 16 axis-aligned quads at z = 0.25 over [-1, 1]^2: shared edges and vertices, zero-thickness boxes (vertices are multiples of 1/8: exact)
    g = []
    for j in range(16):
        for i in range(16):
            x0, x1, y0, y1 = -1 + i / 8, -1 + (i + 1) / 8, -1 + j / 8, -1 + (j + 1) / 8
            g.append([[x0, y0, 0.25], [x1, y0, 0.25], [x1, y1, 0.25]])
            g.append([[x0, y0, 0.25], [x1, y1, 0.25], [x0, y1, 0.25]])
    tris.append(np.array(g))
    # one triangle spanning the whole scene
    tris.append(np.array([[[-1.0, -1.0, -1.0], [1.0, 1.0, -1.0], [-1.0, 1.0, 1.0]]]))
    # 32 slivers of aspect about 1e-5
    a = rng.uniform(-0.8, 0.8, (32, 3))
    u = rng.normal(size=(32, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, rng.normal(size=(32, 3))); w /= np.linalg.norm(w, axis=1, keepdims=True)
    ln = rng.uniform(0.3, 0.6, (32, 1))
    tris.append(np.stack([a, a + ln * u, a + 0.5 * ln * u + 1e-5 * ln * w], 1))
    # 32 degenerate triangles on a 1/64 lattice (exact in float32): 16 with two equal vertices, 16 collinear
    p = rng.integers(-48, 48, (32, 3)) / 64.0
    e = rng.integers(1, 8, (32, 3)) / 64.0
    deg = np.stack([p, p + e, p + 2 * e], 1)
    deg[:16, 1] = deg[:16, 0]
    tris.append(deg)
    t = np.concatenate(tris).astype(F32)
    assert t.shape[0] == 1089
    # 64 exact duplicates of earlier triangles (a BVH4 tests them in slot order, not prim order), half of them of grid triangles
    dup = np.concatenate([rng.choice(512, 24, replace=False), GRID_FIRST + rng.choice(GRID_COUNT, 32, replace=False), 1025 + rng.choice(64, 8, replace=False)])
    t = np.concatenate([t, t[dup]])
    # 32 earlier triangles with reversed winding
    rev = np.concatenate([rng.choice(512, 16, replace=False), GRID_FIRST + rng.choice(GRID_COUNT, 16, replace=False)])
    t = np.concatenate([t, t[rev][:, [0, 2, 1]]])
    assert t.shape == (1185, 3, 3) and t.dtype == F32
    return t


def soup_arrays(translate=(0.0, 0.0, 0.0), seed=20251):
    """Scene arrays (keys of Scene.arrays()) of the soup as one instance under a translation."""
    t = soup_triangles(seed)
    n = t.shape[0]
    mats = np.zeros(1, hjr.MATERIAL_DTYPE)
    mats[0]["basecolor"] = (0.5, 0.5, 0.5)
    mats[0]["roughness"] = 0.5
    mats[0]["ior"] = 1.0
    for k in ("basecolor_tex", "metallic_roughness_tex", "normal_tex", "emission_tex"):
        mats[0][k] = -1
    m = IDENTITY.copy(); inv = IDENTITY.copy()
    m[0, [3, 7, 11]] = translate
    inv[0, [3, 7, 11]] = [-x for x in translate]
    return dict(vertices=t.reshape(-1, 3), normals=np.tile(np.array([[0, 0, 1]], F32), (3 * n, 1)), texcoords=np.zeros((3 * n, 2), F32),
                indices=np.arange(3 * n, dtype=np.uint32), material_ids=np.zeros(n, np.uint32), prim_offsets=np.zeros(1, np.uint32),
                transforms=m, inv_transforms=inv, materials=mats, light_prim_ids=np.zeros(0, np.uint32), light_prim_emission=np.zeros(0, F32))


def world_triangles(arrays):
    """[n, 3, 3] float32 world-space vertices (close to what the builders compute; exact for identity and pure translations)."""
    v = np.asarray(arrays["vertices"], F32).reshape(-1, 3)[np.asarray(arrays["indices"]).reshape(-1)].reshape(-1, 3, 3)
    po = np.asarray(arrays["prim_offsets"]).reshape(-1)
    m = np.asarray(arrays["transforms"], F32).reshape(-1, 3, 4)
    out = np.empty_like(v)
    for i in range(po.size):
        a, b = int(po[i]), int(po[i + 1]) if i + 1 < po.size else v.shape[0]
        r = m[i, :, :3]
        out[a:b] = (v[a:b, :, 0:1] * r[:, 0] + v[a:b, :, 1:2] * r[:, 1] + v[a:b, :, 2:3] * r[:, 2] + m[i, :, 3]).astype(F32)
    return out


class Frame:
    """Where the ray classes live: soup coordinate p maps to centre + scale * p."""

    def __init__(self, arrays, grid=None):
        self.tris = world_triangles(arrays)
        lo, hi = self.tris.reshape(-1, 3).min(0), self.tris.reshape(-1, 3).max(0)
        self.centre = (0.5 * (lo.astype(np.float64) + hi)).astype(F32)
        self.scale = F32(0.5 * float((hi - lo).max()))
        self.max_coord = float(np.abs(self.tris).max())
        self.has_grid = grid is not None
        self.grid = grid if grid is not None else np.arange(self.tris.shape[0])  # triangles the edge / vertex classes aim at (no grid: the scene's own)

    def pt(self, p):
        return (self.centre + self.scale * np.asarray(p, F32)).astype(F32)


# ------------------------------------------------------------------ ray classes (closest-hit rays; [n, 3] origins and directions)
def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def class1_random(fr, rng, n=4000):
    return fr.pt(rng.uniform(-0.95, 0.95, (n, 3))), _unit(rng, n)


TINY = np.array([0.0, -0.0, 1e-38, -1e-38, 1e-31, -1e-31, 1e-29, -1e-29, 1e-20], F32)  # +0, -0, denormal, below / above box_dir's 1e-30 clamp


def class2_axis_parallel(fr, rng, n=1200):
    o = fr.pt(rng.uniform(-0.95, 0.95, (n, 3)))
    d = TINY[rng.integers(0, TINY.size, (n, 3))]
    ax = np.arange(n) % 3
    d[np.arange(n), ax] = np.where(rng.integers(0, 2, n) == 0, F32(1), F32(-1))
    return o, d


def class3_edges_vertices(fr, rng, n=2000):
    """aimed exactly at vertices and edge midpoints of the `grid` triangles, un-normalised: t == 1 at the target"""
    t = fr.tris[rng.choice(fr.grid, n)]
    k = rng.integers(0, 3, n)
    vert = t[np.arange(n), k]
    mid = (F32(0.5) * (vert + t[np.arange(n), (k + 1) % 3])).astype(F32)
    target = np.where((np.arange(n) % 2 == 0)[:, None], vert, mid)
    o = fr.pt(rng.uniform(-0.95, 0.95, (n, 3)))
    return o, (target - o).astype(F32)


def class4_in_plane(fr, rng, n=500):
    """origin and direction inside the grid's plane, built from the edges of grid triangles (axis-aligned: exactly in the plane, every grid
    triangle has det == 0).  A scene without the grid gets the same plane, soup z = 0.25 scaled and translated, as the issue words it.
    (Rays in the plane of an arbitrarily oriented triangle of the scene are NOT a case: there det is rounding noise instead of 0, and the
    float32 ray_tri of product and oracle alike can accept a "hit" far outside the triangle and its box, which no BVH then finds — the
    brute force stops being the ground truth.  DESIGN.md 4.3 has the one such ray that was met.)"""
    if fr.has_grid:
        t = fr.tris[rng.choice(fr.grid, n)]
    else:
        c = rng.uniform(-1, 1, (n, 2))
        t = fr.pt(np.stack([np.stack([c[:, 0], c[:, 1], np.full(n, 0.25)], 1), np.stack([c[:, 0] + 0.125, c[:, 1], np.full(n, 0.25)], 1),
                            np.stack([c[:, 0] + 0.125, c[:, 1] + 0.125, np.full(n, 0.25)], 1)], 1))
        t[:, :, 2] = t[:, 0:1, 2]
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    a, b = rng.uniform(-3, 4, (n, 1)).astype(F32), rng.uniform(-3, 4, (n, 1)).astype(F32)
    c1, c2 = rng.uniform(-1, 1, (n, 1)).astype(F32), rng.uniform(-1, 1, (n, 1)).astype(F32)
    return (t[:, 0] + a * e1 + b * e2).astype(F32), (c1 * e1 + c2 * e2).astype(F32)


def class5_far(fr, rng, factor, n=1500):
    """origins factor x the scene's max |coord| away, aimed at a point inside the scene"""
    target = fr.pt(rng.uniform(-0.8, 0.8, (n, 3)))
    u = _unit(rng, n)
    return (target - F32(factor * fr.max_coord) * u).astype(F32), u


def class8_non_finite(fr, rng, n=64):
    o, d = class1_random(fr, rng, n)
    bad = np.array([np.nan, np.inf, -np.inf], F32)
    for i in range(n):
        (o if (i // 3) % 2 == 0 else d)[i, (i // 6) % 3] = bad[i % 3]
    return o, d


def make_rays(o, d, tmax=None, valid=1):
    r = np.zeros(o.shape[0], hjr.RAY_DTYPE)
    r["o"], r["d"] = o, d
    r["tmax"] = F32(1e16) if tmax is None else tmax
    r["valid"] = valid
    return r


# ------------------------------------------------------------------ ground truth: the oracle's brute force over all triangles
def brute_closest(osc, o, d, tmin=TMIN):
    n = o.shape[0]
    prim = np.full(n, NO_PRIM, np.uint32)
    tb = np.zeros((n, 3), F32)
    for i in range(n):
        p, out = osc.trace_closest(o[i], d[i], tmin, 1e16, use_bvh=0)
        if p >= 0:
            prim[i], tb[i] = p, out
    return prim, tb


def brute_reference(osc, shadow, closest):
    """What hjr_trace_rays must return for the pairs, as RAY_RESULT_DTYPE (k is not part of the reference: left 0)."""
    n = shadow.size
    ref = np.zeros(n, hjr.RAY_RESULT_DTYPE)
    ref["prim"] = NO_PRIM
    for i in range(n):
        if shadow["valid"][i]:
            ref["occluded"][i] = osc.trace_any(shadow["o"][i], shadow["d"][i], TMIN, shadow["tmax"][i], use_bvh=0)
        if closest["valid"][i]:
            p, out = osc.trace_closest(closest["o"][i], closest["d"][i], TMIN, 1e16, use_bvh=0)
            if p >= 0:
                ref["prim"][i], ref["t"][i], ref["b1"][i], ref["b2"][i] = p, out[0], out[1], out[2]
    return ref


def bvh_reference(osc, shadow, closest):
    """The same through the oracle's own BVH (the CPU check that the inputs do not break the oracle itself)."""
    n = shadow.size
    ref = np.zeros(n, hjr.RAY_RESULT_DTYPE)
    ref["prim"] = NO_PRIM
    for i in range(n):
        ref["occluded"][i] = osc.trace_any(shadow["o"][i], shadow["d"][i], TMIN, shadow["tmax"][i], use_bvh=1)
        p, out = osc.trace_closest(closest["o"][i], closest["d"][i], TMIN, 1e16, use_bvh=1)
        if p >= 0:
            ref["prim"][i], ref["t"][i], ref["b1"][i], ref["b2"][i] = p, out[0], out[1], out[2]
    return ref


# ------------------------------------------------------------------ classes that need the ground truth of class 1
def class6_shadow_bounds(o1, d1, prim1, t1, n=500):
    """class-1 rays that hit, as shadow rays ending exactly at the blocker, one ulp behind it, one ulp before it and half way"""
    idx = np.flatnonzero(prim1 != NO_PRIM)[:n]
    t = t1[idx]
    tmax = np.stack([t, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(0)), (F32(0.5) * t).astype(F32)], 1).reshape(-1)
    return np.repeat(o1[idx], 4, 0), np.repeat(d1[idx], 4, 0), tmax


def class7_on_surface(osc, fr, rng, o1, d1, prim1, t1, n=1000, n_tmin=120):
    """hit points of class 1 as origins, and origins whose next surface lies at t = 0.001 exactly / one ulp above / one ulp below (tmin is
    strict).  The latter are found by search: the origin is put 2^-10 scene units before a class-1 hit, and the direction is scaled through
    neighbouring float32 factors until the brute force (tmin = 0) reports the wanted t."""
    idx = np.flatnonzero(prim1 != NO_PRIM)
    h = idx[:n]
    o_hit = (o1[h] + t1[h, None] * d1[h]).astype(F32)
    d_hit = _unit(rng, h.size)
    want = [TMIN, np.nextafter(TMIN, F32(1)), np.nextafter(TMIN, F32(0))]
    oo, dd = [], []
    back = F32(float(fr.scale) / 1024.0)
    for i in idx[idx >= 0][-n_tmin:]:
        if t1[i] <= 4 * back:
            continue
        o = (o1[i] + (t1[i] - back) * d1[i]).astype(F32)
        _, out = osc.trace_closest(o, d1[i], 0.0, 1e16, use_bvh=0)
        s = F32(out[0] / TMIN)
        found = {}
        for _ in range(24):
            s = np.nextafter(s, F32(0))
        for _ in range(49):
            d = (d1[i] * s).astype(F32)
            p, out = osc.trace_closest(o, d, 0.0, 1e16, use_bvh=0)
            for w in want:
                if p >= 0 and out[0] == w and float(w) not in found:
                    found[float(w)] = d
            s = np.nextafter(s, F32(np.inf))
        for d in found.values():
            oo.append(o); dd.append(d)
    n_edge = len(oo)
    o = np.concatenate([o_hit, np.array(oo, F32).reshape(-1, 3)])
    d = np.concatenate([d_hit, np.array(dd, F32).reshape(-1, 3)])
    return o, d, n_edge


# ------------------------------------------------------------------ the batch of a scene
class Batch:
    """Classes 1 - 7 of a scene as pairs (shadow[i], closest[i]) in class order, with the slice of each class, and class 8 apart."""

    def __init__(self, arrays, grid=None, seed=77):
        self.osc = ob.OracleScene(arrays, ob.MATH_PORTABLE)
        fr = self.frame = Frame(arrays, grid)
        rng = np.random.default_rng(seed)
        parts = [("1", class1_random(fr, rng)), ("2", class2_axis_parallel(fr, rng)), ("3", class3_edges_vertices(fr, rng)),
                 ("4", class4_in_plane(fr, rng)), ("5a", class5_far(fr, rng, 8.0)), ("5b", class5_far(fr, rng, 64.0))]
        o1, d1 = parts[0][1]
        prim1, tb1 = brute_closest(self.osc, o1, d1)
        o7, d7, self.n_tmin_edge = class7_on_surface(self.osc, fr, rng, o1, d1, prim1, tb1[:, 0])
        parts.append(("7", (o7, d7)))
        sh, cl, self.slices, at = [], [], {}, 0
        for name, (o, d) in parts:
            n = o.shape[0]
            cl.append(make_rays(o, d))
            # the shadow ray of a pair is another ray of the class, ending somewhere inside the scene
            sh.append(make_rays(np.roll(o, 1, 0), np.roll(d, 1, 0), (rng.uniform(0.02, 2.5, n) * float(fr.scale) / np.maximum(np.linalg.norm(np.roll(d, 1, 0), axis=1), 1e-3)).astype(F32)))
            self.slices[name] = slice(at, at + n); at += n
        o6, d6, tmax6 = class6_shadow_bounds(o1, d1, prim1, tb1[:, 0])
        sh.append(make_rays(o6, d6, tmax6)); cl.append(make_rays(o6, d6))
        self.slices["6"] = slice(at, at + o6.shape[0])
        self.shadow, self.closest = np.concatenate(sh), np.concatenate(cl)
        # the far classes' shadow rays must reach the scene: their tmax spans the distance to it
        for name, k in (("5a", 8.0), ("5b", 64.0)):
            s = self.slices[name]
            self.shadow["tmax"][s] = (rng.uniform(0.5, 1.5, s.stop - s.start) * k * fr.max_coord).astype(F32)
        o8, d8 = class8_non_finite(fr, rng)
        self.shadow8 = make_rays(np.roll(o8, 1, 0), np.roll(d8, 1, 0), F32(2.0) * fr.scale)
        self.closest8 = make_rays(o8, d8)
        self._ref = self._ref8 = None

    @property
    def n(self):
        return self.shadow.size

    @property
    def ref(self):
        if self._ref is None:
            self._ref = brute_reference(self.osc, self.shadow, self.closest)
        return self._ref

    @property
    def ref8(self):
        if self._ref8 is None:
            self._ref8 = brute_reference(self.osc, self.shadow8, self.closest8)
        return self._ref8


def valid_mix(n, seed=5):
    """(shadow valid, closest valid) flags: both, shadow only, closest only, neither, in a fixed pseudo-random order"""
    m = np.random.default_rng(seed).integers(0, 4, n)
    return ((m == 0) | (m == 1)).astype(np.uint32), ((m == 0) | (m == 2)).astype(np.uint32)


def masked_ref(ref, sv, cv):
    r = ref.copy()
    r["occluded"][sv == 0] = 0
    for k in ("t", "b1", "b2"):
        r[k][cv == 0] = 0
    r["prim"][cv == 0] = NO_PRIM
    return r


FIELDS = ("occluded", "prim", "t", "b1", "b2")


def mismatches(got, ref):
    """indices where any compared field differs, bit for bit"""
    bad = np.zeros(got.size, bool)
    for k in FIELDS:
        bad |= got[k].view(np.uint32) != ref[k].view(np.uint32)
    return np.flatnonzero(bad)
