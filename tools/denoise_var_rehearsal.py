#!/usr/bin/env python3
"""CPU rehearsal of the variance-guided filter's two quality conditions, no GPU: frames from the CPU oracle, the native
checker tests/native/denoise_var_ref.cpp as the filter, the oracle's hjo_denoise as the plain filter.

The oracle renders means only, so a frame of N spp is assembled here from N / 8 independent 8-spp oracle frames (frame index k + 1,
one per chunk): chunk sum = 8 x that frame, the frame's mean and its rule-7 variance follow from the chunk sums as in the library.
The frames of 16 / 64 / 256 / 1024 spp are nested (the first 2 / 8 / 32 / 128 chunks).  Reference: 4096 spp, another seed.

    python tools/denoise_var_rehearsal.py [--w 96 --h 64] [--sigma 4 --eps 1e-3] ...
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_binding as ob  # noqa: E402
from denoise_var_util import denoise_var_ref, variance_rule  # noqa: E402
from scene_util import Cornell  # noqa: E402

f32 = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=96)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--cam-x", type=float, default=3.5, help="camera position along its axis (the scene's own camera stands at 5.385622)")
    ap.add_argument("--sigma", type=float, nargs="*", default=[4.0])
    ap.add_argument("--eps", type=float, nargs="*", default=[1e-3])
    a = ap.parse_args()
    w, h = a.w, a.h
    s = Cornell()
    o = ob.OracleScene(s.arrays, ob.MATH_PORTABLE)
    cam = s.camera.as_dict()
    cam["pos"][0] = a.cam_x  # 3.5: the box opening fills the 3:2 frame (from the scene's own position 48 % of it is background)

    def params(spp, frame, seed):
        return ob.make_params(w, h, spp, cam, frame=frame, seed=seed, sky=tuple(s.opt.scene_sky_default), ibl_intensity=s.opt.IBL_intensity)
    ref, _, _, _ = o.render(params(a.ref_spp, 1, 7))
    mask = (ref[..., :3].max(axis=-1) < 3.0) & (np.abs(ref[..., :3] - 0.8).max(axis=-1) > 1e-3)  # lights and background out
    print("mask keeps %.1f %% of the pixels" % (100.0 * mask.mean()))

    def rmse(img):
        return float(np.sqrt(np.mean((img[..., :3][mask].astype(np.float64) - ref[..., :3][mask]) ** 2)))

    spps = (16, 64, 256, 1024)
    chunks = np.zeros((spps[-1] // 8, h, w, 3, 3), f32)
    for k in range(spps[-1] // 8):
        c, al, n, _ = o.render(params(8, k + 1, 1))
        chunks[k] = np.stack([c[..., :3], al[..., :3], n[..., :3]], axis=2) * f32(8)
    frames = {}
    for spp in spps:
        m = spp // 8
        run = np.zeros((h, w, 3, 3), f32)
        for k in range(m):
            run = run + chunks[k]
        img = np.ones((3, h, w, 4), f32)
        img[..., :3] = np.moveaxis(run * (f32(1) / f32(spp)), 2, 0)
        frames[spp] = (img[0], img[1], img[2], variance_rule(chunks[:m, :, :, 0, :], 8, m, spp))
    for sigma in a.sigma:
        for eps in a.eps:
            print("sigma_l %g eps %g" % (sigma, eps))
            prev = None
            ok = True
            for spp in spps:
                c, al, n, v = frames[spp]
                e_raw, e_plain = rmse(c), rmse(ob.denoise(1, c, al, n))
                e_var = rmse(denoise_var_ref(1, c, al, n, v, sigma, eps)[0])
                ok = ok and (spp == 16 or e_var < e_plain) and (prev is None or e_var < prev)
                prev = e_var
                print("  spp %5d  e_raw %.5f  e_plain %.5f  e_var %.5f  e_var/e_raw %.3f" % (spp, e_raw, e_plain, e_var, e_var / e_raw))
            print("  conditions (e_var < e_plain at 64, 256, 1024; e_var strictly decreasing): %s" % ("hold" if ok else "FAIL"))


if __name__ == "__main__":
    main()
