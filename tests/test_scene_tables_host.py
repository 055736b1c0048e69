"""CPU pins of the scene-table tests (tests/test_gpu_scene_tables.py): the generator of tests/table_util.py builds what its options ask
for, and the oracle renders every scene the GPU file uses without NaN samples, with light samples, and differently once the emitters'
transforms are taken away.  The zero-area emitter's NaN samples under MIS, and the channels of the metallic-roughness texture, are
pinned here as well: the GPU tests rely on them."""
import numpy as np
import pytest

import oracle_binding as ob
import table_util as tu

W, H, SPP = 72, 48, 5
NEE, PT, MIS = ob.INTEGRATOR_NEE, ob.INTEGRATOR_PT, ob.INTEGRATOR_MIS


def render(s, integrator):
    return ob.OracleScene(s.arrays, ob.MATH_PORTABLE).render(s.oracle_params(W, H, SPP, integrator=integrator))


def instance_of(a, prim):
    """last instance whose offset is <= prim (an empty instance shares its offset with its successor, which owns the triangles)"""
    return int(np.searchsorted(a["prim_offsets"], prim, side="right")) - 1


# ------------------------------------------------------------------ the generator
def test_generation_is_deterministic():
    a, b = tu.TableScene(seed=5, shuffle=True, duplicate=True).arrays, tu.TableScene(seed=5, shuffle=True, duplicate=True).arrays
    for k in a:
        if k != "textures":
            assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), k
    c = tu.TableScene(seed=6, shuffle=True, duplicate=True).arrays
    assert not np.array_equal(a["vertices"], c["vertices"])


@pytest.mark.parametrize("name", list(tu.SCENES))
def test_counts_offsets_and_materials(name):
    s = tu.scene(name)
    a, info = s.arrays, s.info
    n_floor, n_emit, tri_per = info["n_floor"], info["n_emit"], info["tri_per"]
    extra = 2 if name == "ends" else 0
    n_tris = 2 * n_floor + n_emit * tri_per + extra
    assert info["n_tris"] == n_tris == a["indices"].size // 3 == a["material_ids"].size
    assert a["vertices"].shape == a["normals"].shape == (3 * n_tris, 3) and a["texcoords"].shape == (3 * n_tris, 2)
    n_inst = 1 + n_emit + (1 if name == "empty_before" else 0)
    assert a["prim_offsets"].size == n_inst == a["transforms"].shape[0] == a["inv_transforms"].shape[0]
    assert a["prim_offsets"][0] == 0 and (np.diff(a["prim_offsets"].astype(np.int64)) >= 0).all()
    # every floor patch has a material of its own, every emitter instance an emissive one of its own
    first = info["floor_first_prim"]
    assert np.array_equal(a["material_ids"][first:first + 2 * n_floor], np.repeat(np.arange(n_floor), 2))
    assert (a["vertices"][3 * first:3 * (first + 2 * n_floor), 1] == 0).all()
    mats = a["materials"]
    assert mats.size == n_floor + n_emit + (1 if name == "ends" else 0)
    assert (mats["is_light"][:n_floor] == 0).all() and (mats["is_light"][n_floor:] == 1).all()
    assert set(np.unique(mats["metallic"][:n_floor])) <= set(np.float32(tu.METALLIC))
    assert set(np.unique(mats["roughness"][:n_floor])) <= set(np.float32(tu.ROUGHNESS))
    for e, inst in enumerate(info["emitter_instances"]):
        lo = int(a["prim_offsets"][inst])
        assert (a["material_ids"][lo:lo + tri_per] == n_floor + e).all()
        assert inst + 1 == n_inst or int(a["prim_offsets"][inst + 1]) == lo + tri_per
    assert info["emitter_instances"][-1] == n_inst - 1  # the last instance holds emitters
    # emitter sizes span 0.05 .. 1 in object space (longest edge; a single triangle has size 1)
    if tri_per >= 8:
        lo = int(a["prim_offsets"][info["emitter_instances"][-1]])
        t = a["vertices"][3 * lo:3 * (lo + tri_per)].reshape(-1, 3, 3).astype(np.float64)
        edge = np.linalg.norm(t[:, 1] - t[:, 0], axis=1)
        assert abs(edge.max() - 1.0) < 1e-5 and abs(edge.min() - 0.05) < 1e-5
    # transforms: instance 0 identity, emitters rotated and non-uniformly scaled, every third mirrored, inverse = float64 inverse in float32
    assert np.array_equal(a["transforms"][0], tu.IDENTITY)
    for e, inst in enumerate(info["emitter_instances"]):
        m = a["transforms"][inst].reshape(3, 4).astype(np.float64)
        det = np.linalg.det(m[:, :3])
        assert (det < 0) == (e % 3 == 2), (e, det)
        sv = np.linalg.svd(m[:, :3], compute_uv=False)
        assert 0.3 - 1e-6 <= sv.min() and sv.max() <= 2.0 + 1e-6 and sv.max() / sv.min() > 1.01
        assert abs(m[:, :3] - np.diag(np.diag(m[:, :3]))).max() > 1e-3  # rotated
        inv = np.linalg.inv(np.vstack([m, [0, 0, 0, 1]]))[:3].astype(np.float32).reshape(12)
        assert np.array_equal(inv, a["inv_transforms"][inst])
    # uv across the floor runs from -1.5 to 2.5
    uv = a["texcoords"][3 * first:3 * (first + 2 * n_floor)]
    assert uv[:, 0].min() == np.float32(tu.UV_LO) and uv[:, 0].max() == np.float32(tu.UV_HI) and uv[:, 1].min() == np.float32(tu.UV_LO)


def test_light_lists_are_what_the_options_ask_for():
    def lit(s):
        return np.flatnonzero(s.arrays["materials"]["is_light"][s.arrays["material_ids"]] == 1)
    base = tu.scene("lights64")
    ids = base.arrays["light_prim_ids"]
    assert np.array_equal(ids, lit(base)) and ids.size == 64  # triangle order, every emissive triangle once
    em = base.arrays["materials"]["emission"][base.arrays["material_ids"][ids]]
    assert np.array_equal(base.arrays["light_prim_emission"], em)
    for name, n in tu.LIGHT_COUNTS.items():
        assert tu.scene(name).arrays["light_prim_ids"].size == n
    for name, n in tu.MATERIAL_COUNTS.items():
        assert tu.scene(name).arrays["materials"].size == n
    both = tu.scene("both").arrays
    assert both["light_prim_ids"].size == 200 and both["materials"].size == 210
    assert max(s.info["n_tris"] for s in map(tu.scene, tu.SCENES)) < 1500
    s = tu.scene("shuffled")
    ids = s.arrays["light_prim_ids"]
    assert np.array_equal(np.sort(ids), lit(s)) and (np.diff(ids.astype(np.int64)) < 0).sum() > 16
    assert np.array_equal(s.arrays["light_prim_emission"], s.arrays["materials"]["emission"][s.arrays["material_ids"][ids]])
    s = tu.scene("duplicate")
    ids = s.arrays["light_prim_ids"]
    u, c = np.unique(ids, return_counts=True)
    assert ids.size == 65 and np.array_equal(u, lit(s)) and np.array_equal(u[c == 2], [s.info["duplicate_prim"]]) and (c <= 2).all()
    s = tu.scene("unlisted")
    ids = s.arrays["light_prim_ids"]
    missing = np.setdiff1d(lit(s), ids)
    assert ids.size == 63 and np.array_equal(missing, [s.info["unlisted_prim"]])
    assert s.arrays["materials"]["is_light"][s.arrays["material_ids"][missing[0]]] == 1
    s = tu.scene("odd_emission")
    ids = s.arrays["light_prim_ids"]
    differs = (s.arrays["light_prim_emission"] != s.arrays["materials"]["emission"][s.arrays["material_ids"][ids]]).any(1)
    assert np.array_equal(np.flatnonzero(differs), [s.info["odd_row"]])
    s = tu.scene("ends")
    ids = s.arrays["light_prim_ids"]
    assert ids.size == 66 and ids[0] == 0 and ids[1] == 1 and instance_of(s.arrays, 0) == 0
    assert instance_of(s.arrays, ids.max()) == s.arrays["prim_offsets"].size - 1 and ids.max() == s.info["n_tris"] - 1
    s = tu.scene("empty_before")
    e = s.info["empty_instance"]
    po = s.arrays["prim_offsets"]
    assert po[e] == po[e + 1] and e + 1 in s.info["emitter_instances"] and s.arrays["light_prim_ids"].size == 64
    assert instance_of(s.arrays, int(po[e])) == e + 1  # the triangles at the shared offset belong to the emitter behind the empty instance
    assert not np.array_equal(s.arrays["transforms"][e], s.arrays["transforms"][e + 1])
    s = tu.scene("zero_area")
    t = s.arrays["vertices"].reshape(-1, 3, 3)[s.info["zero_area_prim"]]
    assert np.array_equal(t[0], t[1]) and not np.array_equal(t[0], t[2]) and s.info["zero_area_prim"] in s.arrays["light_prim_ids"]
    s = tu.scene("lights64", pad_materials=37)
    assert s.arrays["materials"].size == 16 + 8 + 37 and s.arrays["material_ids"].max() == 16 + 8 - 1
    assert np.array_equal(tu.scene("lights64").with_padding(37).arrays["materials"], s.arrays["materials"])


# ------------------------------------------------------------------ the oracle on every scene of the GPU file
@pytest.mark.parametrize("name", [n for n in tu.SCENES if n != "zero_area"] + list(tu.TEXTURE_SCENES))
def test_oracle_renders_the_scene_and_the_transforms_matter(name):
    s = tu.scene(name)
    frames = {}
    for integ in (NEE, PT, MIS):
        color, albedo, normal, st = render(s, integ)
        assert st["nan_samples"] == 0 and st["samples"] == W * H * SPP
        assert np.isfinite(color).all() and np.isfinite(albedo).all() and np.isfinite(normal).all()
        assert (st["light_samples"] > 0) if integ != PT else (st["light_samples"] == 0), st  # Pathtrace samples no light
        frames[integ] = color
    flat = tu.scene(name, identity_emitters=True)
    assert np.array_equal(flat.arrays["light_prim_ids"], s.arrays["light_prim_ids"])
    for integ in (NEE, PT, MIS):
        other, _, _, _ = render(flat, integ)
        assert (other != frames[integ]).any(), "the emitters' transforms do not show in the frame"


def test_empty_light_list_with_emissive_surfaces():
    """No light list, but is_light materials: NEE and MIS draw no light sample, and a BSDF-sampled emitter hit under MIS weighs with a
    light pdf of 1 / (area x 0) = inf, so it adds nothing — MIS renders what NEE renders, Pathtrace sees the emitters."""
    s = tu.scene("no_list")
    assert s.arrays["light_prim_ids"].size == 0 and s.arrays["light_prim_emission"].size == 0
    assert (s.arrays["materials"]["is_light"][s.arrays["material_ids"]] == 1).sum() == 64
    frames = {}
    for integ in (NEE, PT, MIS):
        frames[integ], _, _, st = render(s, integ)
        assert st["nan_samples"] == 0 and st["light_samples"] == 0 and np.isfinite(frames[integ]).all()
        assert not np.array_equal(frames[integ], render(tu.scene("no_list", identity_emitters=True), integ)[0])
    assert not np.array_equal(frames[PT], frames[MIS])


def test_padding_materials_are_invisible():
    s = tu.scene("lights64")
    for integ in (NEE, MIS):
        a, _, _, _ = render(s, integ)
        b, _, _, _ = render(s.with_padding(300), integ)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_zero_area_emitter_gives_nan_samples_under_mis_only():
    """A light row of area 0 has pdf = inf: NEE's contribution is x / inf = 0, MIS weighs with inf / (inf + p) = NaN.  The GPU test
    compares the counts, so they must not be zero here."""
    s = tu.scene("zero_area")
    for integ in (NEE, PT):
        color, _, _, st = render(s, integ)
        assert st["nan_samples"] == 0 and np.isfinite(color).all()
    color, _, _, st = render(s, MIS)
    assert 0 < st["nan_samples"] < W * H * SPP // 100 and np.isfinite(color).all(), st  # the guard zeroes them: the frame stays finite


def test_list_shapes_change_the_frame():
    """each light-list option changes what the oracle renders (else its GPU case would check nothing beyond the plain scene)"""
    base = {integ: render(tu.scene("lights64"), integ)[0] for integ in (NEE, MIS)}
    for name in ("shuffled", "duplicate", "unlisted", "odd_emission", "ends", "empty_before", "zero_area"):
        for integ in (NEE, MIS):
            assert not np.array_equal(render(tu.scene(name), integ)[0], base[integ]), (name, integ)


# ------------------------------------------------------------------ material textures
def test_texture_images_and_bindings():
    imgs = tu.texture_images()
    assert [(i.shape[1], i.shape[0]) for i, _ in imgs] == [(1, 1), (3, 5), (64, 2), (17, 17)]
    assert [f for _, f in imgs] == [1, 0, 1, 0] and all(i.dtype == np.uint8 and i.shape[2] == 4 for i, _ in imgs)
    offsets = np.cumsum([0] + [i.shape[0] * i.shape[1] for i, _ in imgs])[:4]
    assert len(set(offsets)) == 4
    for k in (1, 3, 2):  # the images bound to the metallic-roughness slot
        assert (imgs[k][0][..., 1] != imgs[k][0][..., 2]).all()
    g = imgs[1][0][..., 1]
    assert (g == 0).any() and (g == 255).any()
    mats = tu.scene("textured").arrays["materials"][:16]
    bound = set(zip(mats["basecolor_tex"] >= 0, mats["metallic_roughness_tex"] >= 0, mats["normal_tex"] >= 0))
    assert {(False, True, False), (True, True, False), (True, True, True), (False, False, False)} <= bound
    assert ((mats["basecolor_tex"] == mats["metallic_roughness_tex"]) & (mats["basecolor_tex"] >= 0)).any()  # one image in two slots
    assert len(set(mats["metallic_roughness_tex"][mats["metallic_roughness_tex"] >= 0])) == 3
    assert (mats["metallic"] > 0).all() and (mats["roughness"] > 0).all()
    assert (tu.scene("textured_no_mr").arrays["materials"]["metallic_roughness_tex"] == -1).all()


def test_each_channel_of_the_metallic_roughness_image_reaches_the_frame():
    base = {integ: render(tu.scene("textured"), integ)[0] for integ in (NEE, MIS)}
    variants = {"slot unbound": tu.scene("textured_no_mr"), "G changed": tu.texture_scene(mr_g_delta=90), "B changed": tu.texture_scene(mr_b_delta=90)}
    g, b = variants["G changed"].arrays["textures"][1][0], variants["B changed"].arrays["textures"][1][0]
    ref = tu.scene("textured").arrays["textures"][1][0]
    assert (g[..., 1] != ref[..., 1]).all() and np.array_equal(g[..., [0, 2, 3]], ref[..., [0, 2, 3]])
    assert (b[..., 2] != ref[..., 2]).all() and np.array_equal(b[..., [0, 1, 3]], ref[..., [0, 1, 3]])
    frames = {}
    for what, s in variants.items():
        for integ in (NEE, MIS):
            frames[what, integ] = render(s, integ)[0]
            assert (frames[what, integ] != base[integ]).any(axis=-1).mean() > 0.01, (what, integ)
    for integ in (NEE, MIS):  # roughness (G) and metallic (B) act differently
        assert not np.array_equal(frames["G changed", integ], frames["B changed", integ])
