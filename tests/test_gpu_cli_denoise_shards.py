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


def run_both(tmp_path, mode, section, frames):
    """The same render_option.json through the single-process path (image name "a") and through --rank 0 --world 1 ("b")."""
    assert os.path.exists(CLI), "henjou_cli is not built (python __graft_entry__.py)"
    work = tmp_path / "run"
    shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
    ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
    ro["Image"].update(image_width=75, image_height=41, max_spp=12, image_name="a")  # ragged frame: 10 x 6 tiles (DenoiseUpScale2X renders 37 x 20)
    ro["Animation"].update(start_frame=1, end_frame=1 + frames)
    ro["Render_mode"] = mode
    if section:
        ro["Henjou_HIP"] = section
    (work / "render_option.json").write_text(json.dumps(ro))
    p = subprocess.run([CLI, "render_option.json"], cwd=work, capture_output=True, text=True, timeout=300)
    ro["Image"]["image_name"] = "b"
    (work / "render_option.json").write_text(json.dumps(ro))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    q = subprocess.run([CLI, "render_option.json", "--rank", "0", "--world", "1"], cwd=work, capture_output=True, text=True, timeout=300, env=env)
    return work, p, q


@pytest.mark.parametrize("mode,section,frames", [("Denoise", None, 1), ("DenoiseUpScale2X", None, 1), ("Denoise", {"denoise_variance": True}, 1),
                                                 ("Denoise", {"denoise_temporal": True}, 3)],
                         ids=["Denoise", "DenoiseUpScale2X", "Denoise-variance", "Denoise-temporal-3-frames"])
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
