"""The frame loop of hjr_render_file (henjou-renderer_amd/host/frame_loop.hpp) on a GPU: three consecutive frames of the bundled
configuration through henjou_cli, 64 x 64, 16 spp, "passes": 2, so that an output slot is used a second time while the scene update of the
next frame runs.  With "serial_io" and without, plain and in four buckets: byte-identical PNGs, each float4_to_srgb8 of that frame rendered
through Device.render."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from scene_util import ROOT, Cornell, f32_time, hjr

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "henjou-renderer_amd", "henjou_cli")
W, H, SPP, FRAMES = 64, 64, 16, (1, 2, 3)


@pytest.fixture(scope="module")
def want():
    """the three frames' PNG pixels from Device.render, one whole-frame launch each"""
    cornell = Cornell()
    d = hjr.Device(0)
    try:
        d.upload_scene(cornell.scene.view)
        out = []
        for f in FRAMES:
            t = f32_time(f, cornell.opt.fps)
            d.set_transforms(*cornell.scene.transforms(t))
            p = hjr.make_params(W, H, SPP, cornell.scene.camera(cornell.opt, t), frame=f, seed=cornell.opt.seed, integrator=cornell.opt.integrator,
                                sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)
            out.append(hjr.float4_to_srgb8(d.render(p, want_aovs=False)[0])[::-1])
    finally:
        d.close()
    return out


@pytest.mark.parametrize("bucket", [None, [32, 32]], ids=["plain", "buckets"])
def test_serial_and_overlapped_loops_write_the_same_frames(tmp_path, want, bucket):
    assert os.path.exists(CLI), "henjou_cli is not built"
    files = {}
    for serial in (True, False):
        work = tmp_path / ("serial%d" % serial)
        shutil.copytree(os.path.join(hjr.ASSETS, "Model"), work / "Model")
        ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
        ro["Image"].update(image_width=W, image_height=H, max_spp=SPP, image_name="fl")
        ro["Animation"].update(start_frame=FRAMES[0], end_frame=FRAMES[-1] + 1)
        ro["Henjou_HIP"] = dict({"passes": 2, "serial_io": serial}, **({"bucket": bucket} if bucket else {}))
        (work / "render_option.json").write_text(json.dumps(ro))
        p = subprocess.run([CLI, "render_option.json"], cwd=work, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        assert p.stderr.count("2 sample passes") == len(FRAMES), p.stderr
        assert ("4 buckets" in p.stderr) == bool(bucket), p.stderr
        paths = [work / ("fl_%03d.png" % f) for f in FRAMES]
        assert all(q.exists() for q in paths) and not (work / ("fl_%03d.png" % (FRAMES[-1] + 1))).exists()
        files[serial] = paths
    for k, f in enumerate(FRAMES):
        assert files[True][k].read_bytes() == files[False][k].read_bytes(), "frame %d: serial_io changes the file" % f
        got = hjr.load_png(str(files[False][k]))
        assert got.shape == want[k].shape and np.array_equal(got, want[k]), "frame %d: %d pixels differ" % (f, int(np.sum(np.any(got != want[k], axis=-1))))
