"""Host side of the deformation feature (no GPU): the glTF loader's morph sets, default weights and evaluated weight tracks against an
independent reading of a generated glTF (tests/deform_util.py), the "morph_targets" key of the "Henjou_HIP" section, the StatsV7 mirror,
and tests/native/morph_blend_test.cpp, a stand-alone program under AddressSanitizer and UBSan for the host blend and the set validation."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import deform_util as du
from scene_util import ROOT, hjr

GLTF_DIR = os.path.join(hjr.ASSETS, "Model", "test_gltf")


def load(tmp_path, name):
    opt = hjr.load_render_option(os.path.join(hjr.ASSETS, "render_option_c1.json"))
    return hjr.Scene(str(tmp_path), name, opt)


@pytest.fixture(scope="module")
def morphed(tmp_path_factory):
    d = tmp_path_factory.mktemp("morph_gltf")
    desc = du.write_morph_gltf(GLTF_DIR, str(d))
    return d, desc, load(d, "cornell_morph.gltf"), du.read_morph_gltf(os.path.join(str(d), "cornell_morph.gltf"))


def test_loader_morph_sets_and_defaults(morphed):
    d, desc, scene, ref = morphed
    rest = load(GLTF_DIR, "cornelbox.gltf")
    a, b = scene.arrays(), rest.arrays()
    for k in ("vertices", "normals", "indices", "prim_offsets"):
        assert a[k].tobytes() == b[k].tobytes(), "the scene view must stay the rest pose: " + k
    sets, defaults = scene.morph()
    prims = ref["primitives"]
    assert len(prims) >= 2 and len(sets) == len(prims), "the generated mesh has several primitives, one set each"
    assert defaults.tobytes() == ref["defaults"][desc["mesh"]].tobytes() and list(defaults) == [np.float32(x) for x in desc["defaults"]]
    first = None
    for s, p in zip(sets, prims):
        assert s["position_deltas"].tobytes() == p["position_deltas"].tobytes()  # de-indexed exactly as the vertices
        assert (s["normal_deltas"] is None) == (p["normal_deltas"] is None)
        if p["normal_deltas"] is not None:
            assert s["normal_deltas"].tobytes() == p["normal_deltas"].tobytes()
        assert s["first_weight"] == 0, "the primitives of one mesh share its weights"
        first = s["first_vertex"] if first is None else first
        assert s["first_vertex"] == first, "sets follow each other in vertex order"
        first += s["position_deltas"].shape[1]
    assert any(s["normal_deltas"] is not None for s in sets) and any(s["normal_deltas"] is None for s in sets)
    # the sets lie inside the instance of the morphed node
    inst = [i for i, n in enumerate(a["instance_animation_id"]) if n == desc["node"]][0]
    lo, hi = du.instance_vertex_range(a, inst)
    assert sets[0]["first_vertex"] == lo and first == hi
    rs, rw = rest.morph()
    assert rs == [] and rw.size == 0 and rest.morph_weights(0.1).size == 0


def test_loader_weight_track(morphed):
    d, desc, scene, ref = morphed
    (track,) = ref["tracks"]
    defaults = ref["defaults"][track["mesh"]]
    # before time 0, at and between the keys, a time before the first glTF key, at and after the last key
    for t in (-1.0, 0.0, 0.01, 1.0 / 24, 0.05, 0.07, 2.0 / 24, 0.1, 3.0 / 24, 0.19, 0.2, 0.5, 100.0):
        want = du.eval_weight_track(defaults, track["times"], track["values"], t)
        got = scene.morph_weights(t)
        assert got.tobytes() == np.asarray(want, np.float32).tobytes(), (t, got, want)
    assert scene.morph_weights(-1.0).tobytes() == defaults.tobytes()
    assert scene.morph_weights(0.5).tobytes() == np.asarray(track["values"][-1], np.float32).tobytes()
    w = np.zeros(3, np.float32)
    assert hjr.lib().hjr_scene_eval_morph_weights(scene._h, C.c_float(0.0), w.ctypes.data, 3) == -1
    assert b"weight count" in hjr.lib().hjr_last_error()


def test_loader_refuses_what_it_does_not_blend(morphed, tmp_path):
    d, desc, scene, ref = morphed
    g = json.load(open(os.path.join(str(d), "cornell_morph.gltf")))
    open(os.path.join(str(tmp_path), g["buffers"][0]["uri"]), "wb").write(open(os.path.join(str(d), g["buffers"][0]["uri"]), "rb").read())
    prim = g["meshes"][desc["mesh"]]["primitives"][0]

    def refused(edit, words):
        h = json.loads(json.dumps(g))
        edit(h, h["meshes"][desc["mesh"]]["primitives"])
        json.dump(h, open(os.path.join(str(tmp_path), "bad.gltf"), "w"))
        with pytest.raises(hjr.HjrError, match=words):
            load(tmp_path, "bad.gltf")

    refused(lambda h, ps: ps[0]["targets"][0].update({"TEXCOORD_0": prim["targets"][0]["POSITION"]}), "unsupported morph target attribute")
    refused(lambda h, ps: h["accessors"][prim["targets"][0]["POSITION"]].update({"sparse": {"count": 1}}), "non-sparse FLOAT VEC3")
    refused(lambda h, ps: h["accessors"][prim["targets"][0]["POSITION"]].update({"componentType": 5123}), "non-sparse FLOAT VEC3")
    refused(lambda h, ps: ps[1]["targets"].pop(), "different numbers of morph targets")
    refused(lambda h, ps: ps[0]["targets"][0].pop("POSITION"), "without POSITION")
    # TANGENT is ignored
    h = json.loads(json.dumps(g))
    h["meshes"][desc["mesh"]]["primitives"][0]["targets"][0]["TANGENT"] = prim["targets"][0]["POSITION"]
    json.dump(h, open(os.path.join(str(tmp_path), "tangent.gltf"), "w"))
    s2, _ = load(tmp_path, "tangent.gltf").morph()
    assert s2[0]["position_deltas"].tobytes() == scene.morph()[0][0]["position_deltas"].tobytes()


def test_render_option_morph_targets_key(tmp_path):
    """"morph_targets": strict bool, default false, bit 26 of the packed section; no other key's value moves."""
    def parse(extra):
        ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
        ro["Henjou_HIP"] = extra
        p = tmp_path / "ro.json"
        p.write_text(json.dumps(ro))
        return hjr.load_render_option(str(p))
    assert parse({}).device_bvh_opt == 0
    assert parse({"morph_targets": True}).device_bvh_opt == 1 << 26 and parse({"morph_targets": 1}).device_bvh_opt == 1 << 26
    assert parse({"morph_targets": False}).device_bvh_opt == 0
    both = parse({"morph_targets": True, "denoise_temporal_moments": True, "firefly_clamp": 64, "device_bvh_opt": 3})
    assert both.device_bvh_opt == (1 << 26) | (1 << 15) | (64 << 16) | 3
    for bad in (2, "yes", 0.5):
        with pytest.raises(hjr.HjrError, match="morph_targets"):
            parse({"morph_targets": bad})


def test_stats_and_morph_mirrors():
    assert C.sizeof(hjr.StatsV7) == C.sizeof(hjr.StatsV6) + 16
    assert hjr.StatsV7.morph_vertices.offset == C.sizeof(hjr.StatsV6) and hjr.StatsV7.geometry_generation.offset == C.sizeof(hjr.StatsV6) + 8
    assert hjr.StatsV7().struct_size == C.sizeof(hjr.StatsV7)
    assert {"morph_vertices", "geometry_generation", "item_chunks"} <= set(hjr.StatsV7().as_dict())
    assert C.sizeof(hjr.MorphSet) == 32 and C.sizeof(hjr.Morph) == 32 and hjr.Morph().struct_size == 32


def test_morph_blend_native(tmp_path):
    exe = str(tmp_path / "morph_blend_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "native", "morph_blend_test.cpp"), os.path.join(ROOT, "henjou-renderer_amd", "host", "frame.cpp"),
                           "-o", exe, "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "morph_blend_test ok" in p.stdout
