"""Shared by the variance-AOV / variance-guided-filter tests: the native checker of the filter (tests/native/denoise_var_ref.cpp, built
once per process with g++ -ffp-contract=off) and the numpy float32 restatement of the variance rule (include/henjou_hip.h, DESIGN.md §4
rule 7)."""
import os
import subprocess
import tempfile

import numpy as np

from scene_util import ROOT

f32 = np.float32
UNKNOWN = f32(1e30)  # HJR_VARIANCE_UNKNOWN

_exe = None
_dir = None


def checker():
    global _exe, _dir
    if _exe is None:
        _dir = tempfile.TemporaryDirectory(prefix="hjr_dnv_")
        exe = os.path.join(_dir.name, "denoise_var_ref")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "denoise_var_ref.cpp"), "-o", exe])
        _exe = exe
    return _exe


def denoise_var_ref(mode, color, albedo, normal, variance, sigma_l=None, eps=None):
    """The native checker on float4 images [h][w][4] and a variance [h][w]: returns (AOV_Output, filtered variance)."""
    color, albedo, normal = (np.ascontiguousarray(a, f32) for a in (color, albedo, normal))
    variance = np.ascontiguousarray(variance, f32)
    h, w = color.shape[:2]
    assert albedo.shape == normal.shape == (h, w, 4) and variance.shape == (h, w)
    exe = checker()
    src, dst = os.path.join(_dir.name, "in.bin"), os.path.join(_dir.name, "out.bin")
    with open(src, "wb") as f:
        for a in (color, albedo, normal, variance):
            f.write(a.tobytes())
    cmd = [exe, str(w), str(h), str(mode), src, dst]
    if sigma_l is not None:
        cmd += [repr(float(sigma_l)), repr(float(1e-3 if eps is None else eps))]
    subprocess.check_call(cmd)
    raw = np.fromfile(dst, f32)
    ow, oh = (2 * w, 2 * h) if mode == 2 else (w, h)
    assert raw.size == ow * oh * 4 + w * h
    return raw[:ow * oh * 4].reshape(oh, ow, 4), raw[ow * oh * 4:].reshape(h, w)


def variance_rule(chunk_color, g, n_full, n):
    """Rule 7 in numpy float32.  chunk_color: [chunks][...][3] colour sums of the chunks a pixel has received, in chunk order; the first
    n_full of them are full; n: the samples the written mean is over (a number, or an array broadcast over the pixels)."""
    shape = chunk_color.shape[1:-1]
    if n_full < 2:
        return np.full(shape, UNKNOWN, f32)
    S1 = np.zeros(shape, f32)
    S2 = np.zeros(shape, f32)
    for k in range(n_full):
        c = chunk_color[k].astype(f32)
        y = (c[..., 0] + c[..., 1]) + c[..., 2]
        S1 = S1 + y
        S2 = S2 + y * y
    m = f32(n_full)
    q = np.maximum(m * S2 - S1 * S1, f32(0))
    return ((q / (m * (m - f32(1)))) / (f32(g) * np.asarray(n, np.uint32).astype(f32))).astype(f32)
