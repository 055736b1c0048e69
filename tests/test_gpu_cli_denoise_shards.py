"""henjou_cli's per-rank code in Render_mode Denoise / DenoiseUpScale2X (packed colour | albedo | normal | variance per rank -> one ncclGather
-> hjr_denoise_shards_device -> PNG), run as a world of one on the box's single GPU: every PNG must be byte-identical to the single-process
path's (hjr_render_file).  Two ranks need two GPUs (RCCL refuses two ranks on one device); N > 1 is covered on emulated ranks by
tests/test_gpu_denoise_shards.py."""
import json
import os
import shutil
import subprocess

import pytest

from scene_util import ROOT, hjr

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")


ALL_KEYS = {"denoise_temporal": True, "denoise_temporal_coverage": 2, "denoise_variance_spatial": True, "upscale_guided": True, "device_bvh": True,
            "device_bvh_opt": 1, "device_bvh_instances": True, "device_bvh_graft": True, "verbose": True}


def run_both(tmp_path, mode, section, frames, base="render_option_c1.json", **top):
    """The same render_option.json through the single-process path (image name "a") and through --rank 0 --world 1 ("b")."""
    assert os.path.exists(CLI), "henjou_cli is not built (python __graft_entry__.py)"
    work = tmp_path / "run"
    shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
    ro = json.load(open(os.path.join(hjr.ASSETS, base)))
    ro["Image"].update(image_width=75, image_height=41, max_spp=12, image_name="a")  # ragged frame: 10 x 6 tiles (DenoiseUpScale2X renders 37 x 20)
    ro["Animation"].update(start_frame=1, end_frame=1 + frames)
    ro["Render_mode"] = mode
    if section:
        ro["Henjou_HIP"] = section
    for k, v in top.items():
        ro[k].update(v)
    (work / "render_option.json").write_text(json.dumps(ro))
    p = subprocess.run([CLI, "render_option.json"], cwd=work, capture_output=True, text=True, timeout=300)
    ro["Image"]["image_name"] = "b"
    (work / "render_option.json").write_text(json.dumps(ro))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    q = subprocess.run([CLI, "render_option.json", "--rank", "0", "--world", "1"], cwd=work, capture_output=True, text=True, timeout=300, env=env)
    return work, p, q


@pytest.mark.parametrize("mode,section,frames", [("Denoise", None, 1), ("DenoiseUpScale2X", None, 1), ("Denoise", {"denoise_variance": True}, 1),
                                                 ("Denoise", {"denoise_temporal": True}, 3), ("DenoiseUpScale2X", ALL_KEYS, 2)],
                         ids=["Denoise", "DenoiseUpScale2X", "Denoise-variance", "Denoise-temporal-3-frames", "DenoiseUpScale2X-all-keys-2-frames"])
def test_cli_rank_path_denoise_modes_equal_the_single_process_png(tmp_path, mode, section, frames):
    work, p, q = run_both(tmp_path, mode, section, frames)
    assert p.returncode == 0, p.stdout + p.stderr
    assert q.returncode == 0, q.stdout + q.stderr
    pngs = []
    for f in range(1, 1 + frames):
        single = (work / ("a_%03d.png" % f)).read_bytes()
        assert (work / ("b_%03d.png" % f)).read_bytes() == single, "frame %d" % f
        assert hjr.load_png(str(work / ("b_%03d.png" % f))).shape == (41, 75, 4)
        pngs.append(single)
    assert len(set(pngs)) == frames  # (an animation: the frames differ)
    assert q.stderr.count("render + gather + assemble") == frames


def test_cli_rank_path_refuses_denoise_temporal_with_noise_threshold(tmp_path):
    work, p, q = run_both(tmp_path, "Denoise", {"denoise_temporal": True, "noise_threshold": 0.05}, 1)
    for r in (p, q):
        assert r.returncode != 0
        assert "\"denoise_temporal\" cannot be combined with \"noise_threshold\"" in r.stderr
    assert not (work / "b_001.png").exists()


def test_missing_lut_with_a_thin_film_material_ends_both_paths(tmp_path):
    """upload_assets (host/render_job.hpp): a LUT file that is missing while a material is thin-film ends the job with the PNG loader's error,
    on the rank path as in hjr_render_file, and neither writes a PNG."""
    work, p, q = run_both(tmp_path, "Default", None, 1, base="render_option_c3.json", Image={"image_width": 16, "image_height": 16, "max_spp": 1},
                          LUT={"LUT_path": "./LUT/no_such_lut.png"})
    for r in (p, q):
        assert r.returncode != 0, r.stdout + r.stderr
        assert "cannot open ./LUT/no_such_lut.png" in r.stderr
    assert not list(work.glob("*.png"))
