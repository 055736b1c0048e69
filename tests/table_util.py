"""Procedural scenes with large scene tables: many emitter triangles under rotated, non-uniformly scaled and mirrored instances, one
material per floor patch, material textures in every slot of the material row.  tests/test_scene_tables_host.py pins them on the CPU,
tests/test_gpu_scene_tables.py renders them on the GPU against the oracle.  Everything is generated from the seed; float32 throughout
(the keys are those of Scene.arrays())."""
import numpy as np

import oracle_binding as ob
from scene_util import hjr, new_device

F32 = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)
FLOOR_HALF = 6.0            # the floor covers [-6, 6]^2 on y = 0
UV_LO, UV_HI = -1.5, 2.5    # uv across the floor: wrap, negative coordinates and texel boundaries all occur
SKY = (0.02, 0.02, 0.03)    # dark: the emitters dominate
# value sets of tests/test_gpu_scenes.py::test_random_materials_and_cameras
METALLIC = (0.0, 0.3, 0.5, 0.51, 1.0)
ROUGHNESS = (0.0, 0.05, 0.3, 0.7, 1.0)
TEX_KEYS = ("basecolor_tex", "metallic_roughness_tex", "normal_tex", "emission_tex")


def camera():
    """fixed: above the floor at (0, 6, 9), looking at the origin"""
    pos = np.array([0.0, 6.0, 9.0])
    d = -pos / np.linalg.norm(pos)
    right = np.array([1.0, 0.0, 0.0])
    up = np.cross(right, d)
    return {"pos": [float(F32(x)) for x in pos], "dir": [float(F32(x)) for x in d], "up": [float(F32(x)) for x in up],
            "right": [float(F32(x)) for x in right], "f": 1.5}


def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _emitter_transform(rng, i):
    """rotation x non-uniform scale in 0.3 .. 2, every third instance with one negated axis (determinant < 0); [12] float32 and its
    float64 inverse rounded to float32"""
    s = rng.uniform(0.3, 2.0, 3)
    if i % 3 == 2:
        s[int(rng.integers(0, 3))] *= -1.0
    m = np.zeros((4, 4))
    m[:3, :3] = _rotation(rng) @ np.diag(s)
    m[:3, 3] = [rng.uniform(-4.0, 4.0), rng.uniform(2.0, 4.5), rng.uniform(-4.0, 3.0)]
    m[3, 3] = 1.0
    m32 = m[:3].astype(F32)
    m[:3] = m32  # the inverse of the matrix the renderer gets
    return m32.reshape(12), np.linalg.inv(m)[:3].astype(F32).reshape(12)


def _emitter_triangles(rng, n, lo=0.05, hi=1.0):
    """n object-space triangles near the origin, sizes spread geometrically over lo .. hi (the largest first), with per-vertex normals
    (the face normal, perturbed per vertex and normalised)"""
    size = np.geomspace(hi, lo, n) if n > 1 else np.array([hi])
    v0 = rng.uniform(-0.5, 0.5, (n, 3))
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, rng.normal(size=(n, 3))); w /= np.linalg.norm(w, axis=1, keepdims=True)
    th = np.radians(rng.uniform(50, 100, (n, 1)))
    e1 = size[:, None] * u
    e2 = size[:, None] * rng.uniform(0.7, 1.0, (n, 1)) * (np.cos(th) * u + np.sin(th) * w)
    v = np.stack([v0 - (e1 + e2) / 3, v0 - (e1 + e2) / 3 + e1, v0 - (e1 + e2) / 3 + e2], 1)
    fn = np.cross(e1, e2); fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    nn = fn[:, None, :] + rng.uniform(-0.2, 0.2, (n, 3, 3))
    nn /= np.linalg.norm(nn, axis=2, keepdims=True)
    return v.astype(F32), nn.astype(F32)


def _blank_materials(n):
    mats = np.zeros(n, hjr.MATERIAL_DTYPE)
    mats["basecolor"] = 0.5
    mats["roughness"] = 0.5
    mats["ior"] = 1.0
    for k in TEX_KEYS:
        mats[k] = -1
    return mats


def _padding(k):
    """k materials no triangle refers to: 80 bytes of the LDS budget each, emissive so that a row read by mistake would show"""
    rng = np.random.default_rng(k)
    pad = _blank_materials(k)
    pad["basecolor"] = rng.uniform(0.0, 1.0, (k, 3)).astype(F32)
    pad["emission"] = rng.uniform(0.0, 9.0, (k, 3)).astype(F32)
    pad["is_light"] = 1
    return pad


class TableScene:
    """The scene: arrays (keys of Scene.arrays()), the fixed camera, and the description the host tests check (`info`).

    Instance 0 is the floor: n_floor quad patches on y = 0, each with its own material (materials 0 .. n_floor - 1).  Instances 1 ..
    n_emit hold tri_per emissive triangles each, every instance with its own emissive material (n_floor + i) and transform.  The
    materials of further emitters and the padding follow.  Options (each on its own):
      empty_before   an instance without triangles (and a transform of its own) in front of emitter instance n_emit // 2
      ends           two more emissive triangles at the START of instance 0 (prims 0 and 1; identity transform); the last instance
                     holds emitters in every scene
      shuffle        the light list in a random order instead of triangle order
      duplicate      one emissive triangle listed twice
      unlisted       the largest triangle of emitter instance 0 keeps its is_light material and is left out of the list
      odd_emission   one row of light_prim_emission differs from the emission of the triangle's material
      zero_area      the last triangle of emitter instance 0 has two equal vertices (it stays in the list)
      pad_materials  k unreferenced materials appended to the table
      empty_list     the light list is empty although the emitters keep their is_light materials
      identity_emitters  every transform is the identity (the host test's counter-example: the transforms matter)"""

    def __init__(self, seed=1, n_floor=16, n_emit=8, tri_per=8, empty_before=False, ends=False, shuffle=False, duplicate=False,
                 unlisted=False, odd_emission=False, zero_area=False, pad_materials=0, identity_emitters=False, empty_list=False):
        rng = np.random.default_rng([seed, n_floor, n_emit, tri_per])
        verts, norms, uvs, mat_ids, prim_offsets, xf, ixf = [], [], [], [], [], [], []
        info = self.info = dict(n_floor=n_floor, n_emit=n_emit, tri_per=tri_per, emitter_instances=[], empty_instance=None)
        n_mats = n_floor + n_emit + (1 if ends else 0)
        mats = _blank_materials(n_mats)
        for i in range(n_floor):
            mats[i]["basecolor"] = rng.uniform(0.05, 1.0, 3).astype(F32)
            mats[i]["metallic"] = F32(rng.choice(METALLIC))
            mats[i]["roughness"] = F32(rng.choice(ROUGHNESS))
        for i in range(n_floor, n_mats):
            mats[i]["emission"] = rng.uniform(2.0, 20.0, 3).astype(F32)
            mats[i]["is_light"] = 1
        n_tris = 0
        lights = []  # (prim, material)
        # ---- instance 0: [emitters of `ends`], floor
        prim_offsets.append(0); xf.append(IDENTITY); ixf.append(IDENTITY)
        if ends:
            v, nn = _emitter_triangles(rng, 2, 0.4, 0.9)
            v = v + np.array([[[-2.5, 1.5, 1.0]], [[2.5, 2.0, 0.5]]], F32)
            verts.append(v.reshape(-1, 3)); norms.append(nn.reshape(-1, 3)); uvs.append(np.zeros((6, 2), F32))
            mat_ids += [n_mats - 1] * 2
            lights += [(0, n_mats - 1), (1, n_mats - 1)]
            n_tris += 2
        cols = int(np.ceil(np.sqrt(n_floor)))
        rows = (n_floor + cols - 1) // cols
        xs = (-FLOOR_HALF + 2 * FLOOR_HALF * np.arange(cols + 1) / cols).astype(F32)
        zs = (-FLOOR_HALF + 2 * FLOOR_HALF * np.arange(rows + 1) / rows).astype(F32)
        us = (UV_LO + (UV_HI - UV_LO) * np.arange(cols + 1) / cols).astype(F32)
        vs = (UV_LO + (UV_HI - UV_LO) * np.arange(rows + 1) / rows).astype(F32)
        info["floor_first_prim"] = n_tris
        for k in range(n_floor):
            i, j = k % cols, k // cols
            p = [(xs[i], zs[j], us[i], vs[j]), (xs[i + 1], zs[j], us[i + 1], vs[j]), (xs[i + 1], zs[j + 1], us[i + 1], vs[j + 1]),
                 (xs[i], zs[j + 1], us[i], vs[j + 1])]
            for a, b, c in ((0, 2, 1), (0, 3, 2)):  # wound so that the face looks up
                verts.append(np.array([[p[q][0], 0.0, p[q][1]] for q in (a, b, c)], F32))
                uvs.append(np.array([[p[q][2], p[q][3]] for q in (a, b, c)], F32))
                norms.append(np.tile(np.array([[0, 1, 0]], F32), (3, 1)))
                mat_ids.append(k)
            n_tris += 2
        # ---- emitter instances
        for e in range(n_emit):
            if empty_before and e == n_emit // 2:
                m, inv = _emitter_transform(rng, 2)  # a mirrored one: picking it by mistake shows
                info["empty_instance"] = len(prim_offsets)
                prim_offsets.append(n_tris); xf.append(m); ixf.append(inv)
            m, inv = _emitter_transform(rng, e)
            info["emitter_instances"].append(len(prim_offsets))
            prim_offsets.append(n_tris); xf.append(m); ixf.append(inv)
            v, nn = _emitter_triangles(rng, tri_per)
            if zero_area and e == 0:
                v[-1, 1] = v[-1, 0]
                info["zero_area_prim"] = n_tris + tri_per - 1
            verts.append(v.reshape(-1, 3)); norms.append(nn.reshape(-1, 3)); uvs.append(np.zeros((3 * tri_per, 2), F32))
            mat_ids += [n_floor + e] * tri_per
            lights += [(n_tris + t, n_floor + e) for t in range(tri_per)]
            n_tris += tri_per
        if unlisted:
            first = info["emitter_instances"][0]
            info["unlisted_prim"] = int(prim_offsets[first])  # the largest triangle of emitter instance 0
            lights = [l for l in lights if l[0] != info["unlisted_prim"]]
        if empty_list:
            lights = []
        if duplicate:
            k = len(lights) // 3
            info["duplicate_prim"] = lights[k][0]
            lights.insert(2 * len(lights) // 3, lights[k])
        if shuffle:
            lights = [lights[i] for i in rng.permutation(len(lights))]
        emission = np.array([mats[m]["emission"] for _, m in lights], F32).reshape(-1, 3)
        if odd_emission:
            k = len(lights) // 2
            info["odd_row"] = k
            emission[k] = emission[k][::-1] * F32(1.5) + F32(0.25)
        if pad_materials:
            mats = np.concatenate([mats, _padding(pad_materials)])
        n_inst = len(prim_offsets)
        if identity_emitters:
            xf = [IDENTITY] * n_inst; ixf = [IDENTITY] * n_inst
        self.camera = camera()
        self.arrays = dict(vertices=np.concatenate(verts).astype(F32), normals=np.concatenate(norms).astype(F32),
                           texcoords=np.concatenate(uvs).astype(F32), indices=np.arange(3 * n_tris, dtype=np.uint32),
                           material_ids=np.array(mat_ids, np.uint32), prim_offsets=np.array(prim_offsets, np.uint32),
                           transforms=np.stack(xf).astype(F32), inv_transforms=np.stack(ixf).astype(F32), materials=mats,
                           light_prim_ids=np.array([p for p, _ in lights], np.uint32), light_prim_emission=emission, textures=[])
        info["n_tris"], info["n_instances"], info["n_referenced_materials"] = n_tris, n_inst, n_mats

    # the surface of scene_util.Cornell the GPU tests use
    def hjr_params(self, w, h, spp, **kw):
        kw.setdefault("sky", SKY)
        return hjr.make_params(w, h, spp, self.camera, **kw)

    def oracle_params(self, w, h, spp, **kw):
        kw.setdefault("sky", SKY)
        return ob.make_params(w, h, spp, self.camera, **kw)

    def device(self, options=None):
        d = new_device(options)
        try:
            d.upload_arrays(self.arrays)
            d.set_transforms(self.arrays["transforms"], self.arrays["inv_transforms"])
        except Exception:
            d.close()
            raise
        return d

    def with_padding(self, k):
        """the same scene with k unreferenced materials appended (shares every other array)"""
        import copy
        s = copy.copy(self)
        s.arrays = dict(self.arrays)
        s.arrays["materials"] = np.concatenate([self.arrays["materials"], _padding(k)])
        return s


# ------------------------------------------------------------------ material textures in every slot of the material row
def texture_images(mr_g_delta=0, mr_b_delta=0):
    """Four generated RGBA8 images of unlike shapes, (pixels [h, w, 4], srgb flag), in atlas order (descriptor offsets 0, 1, 16, 144):
      0  1 x 1   sRGB    a constant base colour
      1  3 x 5   linear  metallic-roughness: G and B differ in every texel, G takes 0 and 255
      2  64 x 2  sRGB    base colour stripes (bound to two slots of one material as well)
      3  17 x 17 linear  a wavy tangent-space normal map (also read as a metallic-roughness image: its G and B differ)
    mr_g_delta / mr_b_delta are added (mod 256) to the G / B channel of image 1 only (the host test's channel pins)."""
    i0 = np.array([[[200, 120, 60, 255]]], np.uint8)
    yy, xx = np.mgrid[0:5, 0:3]
    g = (np.array([0, 255, 37, 128, 90, 200, 255, 0, 64, 180, 15, 240, 100, 220, 5], np.int64).reshape(5, 3) + mr_g_delta) % 256
    b = ((40 + 53 * xx + 29 * yy) % 256 + mr_b_delta) % 256
    i1 = np.stack([np.full((5, 3), 77), g, b, np.full((5, 3), 255)], -1).astype(np.uint8)
    yy, xx = np.mgrid[0:2, 0:64]
    i2 = np.stack([(xx * 4 + 3) % 256, (xx * 37 + yy * 90) % 256, 255 - (xx * 3) % 256, np.full((2, 64), 255)], -1).astype(np.uint8)
    yy, xx = np.mgrid[0:17, 0:17]
    nx = 0.35 * np.sin(xx * 0.9) * np.cos(yy * 0.5)
    ny = 0.35 * np.cos(xx * 0.4 + yy * 0.7)
    nz = np.sqrt(1.0 - nx * nx - ny * ny)
    i3 = np.stack([(nx * 0.5 + 0.5) * 255, (ny * 0.5 + 0.5) * 255, (nz * 0.5 + 0.5) * 255, np.full((17, 17), 255.0)], -1).round().astype(np.uint8)
    return [(i0, 1), (i1, 0), (i2, 1), (i3, 0)]


# bindings of the floor materials, in turn: (basecolor_tex, metallic_roughness_tex, normal_tex)
TEX_BINDINGS = [(-1, 1, -1),   # metallic-roughness only
                (2, 3, -1),    # base colour and metallic-roughness
                (0, 1, 3),     # base colour, metallic-roughness and a normal map on one material
                (2, 2, -1),    # one image bound to two slots of one material
                (-1, -1, -1)]  # untextured


def texture_scene(seed=3, mr_bound=True, mr_g_delta=0, mr_b_delta=0, identity_emitters=False):
    """A 16-patch floor under 64 emitter triangles whose floor materials cycle through TEX_BINDINGS; metallic and roughness factors of
    the textured materials are non-zero so that both texel channels act.  mr_bound=False: the same scene with every
    metallic-roughness slot set to -1."""
    s = TableScene(seed=seed, n_floor=16, n_emit=8, tri_per=8, identity_emitters=identity_emitters)
    mats = s.arrays["materials"]
    rng = np.random.default_rng(seed + 100)
    for i in range(16):
        bc, mr, nm = TEX_BINDINGS[i % len(TEX_BINDINGS)]
        mats[i]["basecolor_tex"], mats[i]["normal_tex"] = bc, nm
        mats[i]["metallic_roughness_tex"] = mr if mr_bound else -1
        mats[i]["metallic"] = F32(rng.choice(METALLIC[1:]))
        mats[i]["roughness"] = F32(rng.choice(ROUGHNESS[2:]))
    s.arrays["textures"] = texture_images(mr_g_delta, mr_b_delta)
    return s


# ------------------------------------------------------------------ the scenes of the tests, by name
# light counts: one row, an odd count, one wave's worth, the first count whose staging loop takes a second trip (171 rows x 6 float4 >
# 1024), and past it; material counts: 2, 65, the first count with a second staging trip (205 rows x 5 float4 > 1024), and past it
SCENES = {
    "lights1": dict(n_floor=4, n_emit=1, tri_per=1),
    "lights3": dict(n_floor=4, n_emit=3, tri_per=1),
    "lights64": dict(n_floor=16, n_emit=8, tri_per=8),
    "lights171": dict(n_floor=16, n_emit=9, tri_per=19),
    "lights200": dict(n_floor=16, n_emit=8, tri_per=25),
    "shuffled": dict(shuffle=True),
    "duplicate": dict(duplicate=True),
    "unlisted": dict(unlisted=True),
    "odd_emission": dict(odd_emission=True),
    "ends": dict(ends=True),
    "empty_before": dict(empty_before=True),
    "zero_area": dict(zero_area=True),
    "mats2": dict(n_floor=1, n_emit=1, tri_per=8),
    "mats65": dict(n_floor=57),
    "mats205": dict(n_floor=197),
    "mats210": dict(n_floor=202),
    "both": dict(n_floor=202, n_emit=8, tri_per=25),  # 200 lights and 210 materials: both tables past one staging trip
}
LIGHT_COUNTS = {"lights1": 1, "lights3": 3, "lights64": 64, "lights171": 171, "lights200": 200}
MATERIAL_COUNTS = {"mats2": 2, "mats65": 65, "mats205": 205, "mats210": 210}
TEXTURE_SCENES = {"textured": dict(), "textured_no_mr": dict(mr_bound=False)}
# MIS with emissive surfaces and no light list: the light pdf of a BSDF-sampled emitter hit is 1 / (area x 0) = inf, its weight 0
OTHER_SCENES = {"no_list": dict(empty_list=True)}
_scenes = {}


def scene(name, **more):
    """the named scene, built once (with `more`: a variant of it, not cached)"""
    def build(**kw):
        if name in TEXTURE_SCENES:
            return texture_scene(**dict(TEXTURE_SCENES[name], **kw))
        return TableScene(**dict(SCENES[name] if name in SCENES else OTHER_SCENES[name], **kw))
    if more:
        return build(**more)
    if name not in _scenes:
        _scenes[name] = build()
    return _scenes[name]
