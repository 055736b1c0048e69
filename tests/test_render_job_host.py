"""The job setup of a render_option.json (henjou-renderer_amd/host/render_job.hpp), without a GPU: the parser against the
recorded results of the hand-written one it replaced, the header's stand-alone program, and the refusals through both drivers."""
import ctypes as C
import json
import os
import subprocess

import pytest

from scene_util import ROOT, hjr

GOLDEN = os.path.join(ROOT, "tests", "golden", "render_option_sections.json")
ERR_ARG = -1


def _option_json(tmp_path, section):
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    if section is not None:
        ro["Henjou_HIP"] = section
    path = tmp_path / "render_option.json"
    path.write_text(json.dumps(ro))
    return str(path)


def test_parser_gives_the_recorded_results(tmp_path, monkeypatch):
    """tests/golden/render_option_sections.json: what hjr_load_render_option gave for each "Henjou_HIP" section before the key table, the
    stored fields or the full error text.  The table walk must give the same fields and byte-equal texts (which of two bad keys is reported
    included)."""
    monkeypatch.chdir(tmp_path)  # (the loader reads ./fps.txt)
    entries = json.load(open(GOLDEN))
    assert len(entries) > 150
    for e in entries:
        opt = hjr.RenderOption()
        rc = hjr.lib().hjr_load_render_option(os.fsencode(_option_json(tmp_path, e["section"])), C.byref(opt))
        if "error" in e:
            assert rc != 0 and hjr.lib().hjr_last_error().decode() == e["error"], (e, rc, hjr.lib().hjr_last_error())
        else:
            assert rc == 0, (e, hjr.lib().hjr_last_error())
            assert {f: getattr(opt, f) for f in e["values"]} == e["values"], e


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("job") / "render_job_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "native", "render_job_test.cpp"), "-o", out,
                           "-L" + hjr.PKG_DIR, "-lhenjou_hip", "-Wl,-rpath," + hjr.PKG_DIR, "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def test_render_job_header_native(native):
    """tests/native/render_job_test.cpp: the table's layout, the option lists of the three scopes, the refusals and the pass split."""
    assert "render_job_test ok" in native


def test_pass_ends_are_pass_bounds(native):
    """The program prints pass_ends for a small grid; hjr.pass_bounds (what the GPU tests of "passes" split by) must agree."""
    lines = [ln.split() for ln in native.splitlines() if ln.startswith("ends ")]
    assert len(lines) >= 40
    for ln in lines:
        spp, passes, ends = int(ln[1]), int(ln[2]), list(map(int, ln[3:]))
        assert [e for _, e in hjr.pass_bounds(spp, passes)] == ends, (spp, passes)


REFUSALS = [
    ("Render_mode", {}, {"Render_mode": "Debug"}, {}),
    ("denoise_temporal", {"denoise_temporal": True, "noise_threshold": 0.05}, {"Render_mode": "Denoise"}, {}),
    ("firefly_clamp", {"firefly_clamp": 4, "passes": 2}, {}, {}),
    ("too small", {}, {"Render_mode": "DenoiseUpScale2X"}, {"image_width": 1, "image_height": 1}),
    # two at once: the earlier one of job_check's order
    ("denoise_temporal", {"denoise_temporal": True, "noise_threshold": 0.05, "firefly_clamp": 4}, {"Render_mode": "DenoiseUpScale2X"}, {"image_width": 1, "image_height": 9}),
]


@pytest.mark.parametrize("word, section, top, image", REFUSALS)
def test_refusals_reach_both_drivers(tmp_path, word, section, top, image):
    """Each refusal of job_check through hjr_render_file (HJR_ERR_ARG) and through the rank path of henjou_cli (exit 1): the same text after
    the driver's own prefix, before the scene is loaded (the glTF named here does not exist) and before any device call (no GPU here)."""
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro.update(top)
    ro["Henjou_HIP"] = section
    ro["Image"].update(image)
    ro["GLTF_file"]["gltf_filename"] = "no_such_scene.gltf"
    path = tmp_path / "x.json"
    path.write_text(json.dumps(ro))
    rc = hjr.lib().hjr_render_file(os.fsencode(str(path)), 0)
    err = hjr.lib().hjr_last_error().decode()
    assert rc == ERR_ARG, (rc, err)
    assert err.startswith("hjr_render_file: ") and word in err and "no_such_scene" not in err
    p = subprocess.run([os.path.join(hjr.PKG_DIR, "henjou_cli"), str(path), "--rank", "0", "--world", "1"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 1, (p.returncode, p.stderr[-800:])
    said = [ln for ln in p.stderr.splitlines() if ln.startswith("henjou_cli: ")]
    assert len(said) == 1 and "no_such_scene" not in p.stderr, p.stderr[-800:]
    assert said[0][len("henjou_cli: "):] == err[len("hjr_render_file: "):]
