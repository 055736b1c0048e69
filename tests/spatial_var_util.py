"""Shared by the spatial-variance-estimate tests and tools: the native checker of the estimate (tests/native/spatial_var_ref.cpp, built once
per process with g++ -O2 -ffp-contract=off; it restates the header comment of csrc/hjr_denoise.hip.h), and the quality comparison of
DESIGN.md §11.3 on frames from any source (the CPU oracle in tools/spatial_var_rehearsal.py, the GPU in tests/test_gpu_spatial_var.py and
tools/spatial_var_bench.py): every filter stage is a CPU checker, so equal frames give equal tables."""
import os
import subprocess
import tempfile

import numpy as np

import oracle_binding as ob
from denoise_var_util import denoise_var_ref
from scene_util import ROOT, hjr
from temporal_util import camera_at, moved_consistent, ref_mask, rmse, temporal_ref

f32 = np.float32
UNKNOWN = f32(1e30)  # HJR_VARIANCE_UNKNOWN
SPPS = (1, 2, 4, 8)  # every frame of these sample counts is a single chunk: the variance AOV is unknown everywhere
FRAMES, CHAIN_FRAMES, CHAIN_SPP = 4, 8, 4

_exe = None
_dir = None


def checker():
    global _exe, _dir
    if _exe is None:
        _dir = tempfile.TemporaryDirectory(prefix="hjr_spv_")
        exe = os.path.join(_dir.name, "spatial_var_ref")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "spatial_var_ref.cpp"), "-o", exe])
        _exe = exe
    return _exe


def spatial_var_ref(color, albedo, normal, variance=None, radius=None):
    """The native checker on float4 images [h][w][4] and an input variance [h][w] (None = every pixel unknown): the variance [h][w]."""
    color, albedo, normal = (np.ascontiguousarray(a, f32) for a in (color, albedo, normal))
    h, w = color.shape[:2]
    assert color.shape == albedo.shape == normal.shape == (h, w, 4)
    exe = checker()
    src, dst = os.path.join(_dir.name, "in.bin"), os.path.join(_dir.name, "out.bin")
    with open(src, "wb") as f:
        for a in (color, albedo, normal):
            f.write(a.tobytes())
        if variance is not None:
            variance = np.ascontiguousarray(variance, f32)
            assert variance.shape == (h, w)
            f.write(variance.tobytes())
    cmd = [exe, str(w), str(h), "0" if variance is None else "1", src, dst]
    if radius is not None:
        cmd.append(str(int(radius)))
    subprocess.check_call(cmd)
    raw = np.fromfile(dst, f32)
    assert raw.size == w * h
    return raw.reshape(h, w)


def hostile_variance(h, w, seed=5):
    """A checkerboard of known values and unknown pixels: the known half cycles through ordinary variances and the values the pass-through
    rule has to get right (0, negative, NaN, -Inf, 0.999e30: kept as stored) or treat as unknown (+Inf, 1e30, 2e30)."""
    rng = np.random.default_rng(seed)
    v = np.full((h, w), UNKNOWN, f32)
    special = np.array([0.0, -1.0, np.nan, np.inf, 1e30, 0.999e30, -np.inf, 2e30, 1e-3, 0.25], f32)
    yy, xx = np.mgrid[0:h, 0:w]
    known = (yy + xx) % 2 == 0
    k = np.flatnonzero(known.reshape(-1))
    vals = special[np.arange(k.size) % special.size].copy()
    plain = np.arange(k.size) % 3 == 2  # every third known pixel: an ordinary variance
    vals[plain] = rng.uniform(0.0, 0.5, int(plain.sum())).astype(f32)
    v.reshape(-1)[k] = vals
    return v


# ---- the quality comparison
def lower_median(e):
    """Rank 1 of four values in ascending order (the lower median, as the firefly clamp defines it)."""
    return sorted(e)[(len(e) - 1) // 2]


def single_frame_table(get_frame, ref, spps=SPPS, frames=FRAMES, radius=None):
    """get_frame(spp, frame) -> (colour, albedo, normal) of a frame whose variance is unknown everywhere.  Per spp, lists over the frames
    1..frames of the RMSE against `ref` over its mask: the raw frame, the plain filter, the variance-guided filter with the variance
    unknown (what the option off gives), and the variance-guided filter behind the spatial estimate."""
    mask = ref_mask(ref)
    t = {}
    for spp in spps:
        row = {"e_raw": [], "e_plain": [], "e_unknown": [], "e_spatial": []}
        for f in range(1, frames + 1):
            c, a, n = get_frame(spp, f)
            unknown = np.full(c.shape[:2], UNKNOWN, f32)
            row["e_raw"].append(rmse(c, ref, mask))
            row["e_plain"].append(rmse(ob.denoise(1, c, a, n), ref, mask))
            row["e_unknown"].append(rmse(denoise_var_ref(1, c, a, n, unknown)[0], ref, mask))
            row["e_spatial"].append(rmse(denoise_var_ref(1, c, a, n, spatial_var_ref(c, a, n, None, radius))[0], ref, mask))
        t[spp] = row
    return t


def temporal_chain(get_frame, refs, n_tris, radius=None):
    """get_frame(frame) -> (colour, albedo, normal, side) of frames 1..len(refs) at CHAIN_SPP, `side` the dict of camera, transforms,
    inv_transforms and gbuffer that temporal_ref takes.  Per frame the RMSE against refs[frame - 1]: the plain filter without any history,
    the temporal path with the variance unknown (the option off) and the temporal path behind the spatial estimate."""
    t = {"e_plain": [], "e_off": [], "e_on": []}
    prev = {"e_off": None, "e_on": None}
    for f, ref in enumerate(refs, 1):
        mask = ref_mask(ref)
        c, a, n, side = get_frame(f)
        t["e_plain"].append(rmse(ob.denoise(1, c, a, n), ref, mask))
        for key in ("e_off", "e_on"):
            v = np.full(c.shape[:2], UNKNOWN, f32) if key == "e_off" else spatial_var_ref(c, a, n, None, radius)
            cur = dict(side, color=c, variance=v)
            tc, tv, th = temporal_ref(prev[key], cur, n_tris)
            t[key].append(rmse(denoise_var_ref(1, tc, a, n, tv)[0], ref, mask))
            prev[key] = dict(cur, color=tc, variance=tv, history=th)
    return t


# the GPU's frames for the two tables (tests/test_gpu_spatial_var.py, tools/spatial_var_bench.py): 96 x 64, NEE, seed 1, camera at x = 3.5,
# references of 4096 spp with seed 7
QW, QH, REF_SPP = 96, 64, 4096


def _sky(cornell):
    return dict(sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)


def gpu_single_frame_table(cornell, dev):
    cam = camera_at(cornell, x=3.5)
    ref = dev.render(hjr.make_params(QW, QH, REF_SPP, cam, seed=7, **_sky(cornell)), want_aovs=False)[0]
    return single_frame_table(lambda spp, f: dev.render(hjr.make_params(QW, QH, spp, cam, frame=f, seed=1, **_sky(cornell))), ref)


def gpu_temporal_chain(cornell, dev, moving):
    """The 8-frame chain at CHAIN_SPP, `frame` advancing; moving: every instance moved by frame * (0.05, -0.03, 0.02), one reference per
    frame.  Leaves the scene's own transforms current."""
    cam = camera_at(cornell, x=3.5)
    n_tris = np.asarray(cornell.arrays["indices"]).size // 3
    refs, frames = [], {}
    try:
        for f in range(1, CHAIN_FRAMES + 1):
            xf = moved_consistent(cornell.arrays, f if moving else 0)
            if moving or f == 1:
                dev.set_transforms(*xf)
                ref = dev.render(hjr.make_params(QW, QH, REF_SPP, cam, seed=7, **_sky(cornell)), want_aovs=False)[0]
                g = dev.gbuffer(hjr.make_params(QW, QH, 1, cam))
            refs.append(ref)
            side = {"camera": cam, "transforms": xf[0], "inv_transforms": xf[1], "gbuffer": g}
            frames[f] = dev.render(hjr.make_params(QW, QH, CHAIN_SPP, cam, frame=f, seed=1, **_sky(cornell))) + (side,)
    finally:
        dev.set_transforms(cornell.arrays["transforms"], cornell.arrays["inv_transforms"])
    return temporal_chain(lambda f: frames[f], refs, n_tris)


def quality_conditions(table=None, chains=None):
    """The asserted conditions as (text, holds) pairs.  Single frames, with e the lower median of the four frames: e_spatial < e_plain and
    e_spatial < e_unknown at every spp of the table.  Temporal chains ({"static": ..., "moving": ...}): e_on < e_off at every frame."""
    c = []
    for spp, row in sorted((table or {}).items()):
        es, ep, eu = lower_median(row["e_spatial"]), lower_median(row["e_plain"]), lower_median(row["e_unknown"])
        c.append(("%d spp: e_spatial %.5f < e_plain %.5f" % (spp, es, ep), es < ep))
        c.append(("%d spp: e_spatial %.5f < e_unknown %.5f" % (spp, es, eu), es < eu))
    for name, t in sorted((chains or {}).items()):
        for f, (on, off) in enumerate(zip(t["e_on"], t["e_off"]), 1):
            c.append(("%s chain, frame %d: e(temporal + estimate) %.5f < e(temporal, option off) %.5f" % (name, f, on, off), on < off))
    return c


def beats_plain_share(chains):
    """Reported, not asserted: the share of the chains' frames from frame 2 on whose temporal + estimate error is below the plain filter's."""
    wins = [on < pl for t in chains.values() for on, pl in list(zip(t["e_on"], t["e_plain"]))[1:]]
    return float(np.mean(wins)) if wins else 0.0


def format_tables(table=None, chains=None):
    lines = []
    if table:
        lines.append("spp   plain filter (frames 1..%d)          variance-guided, unknown            variance-guided + estimate" % len(next(iter(table.values()))["e_plain"]))
        for spp, row in sorted(table.items()):
            lines.append("%3d   %s   %s   %s" % (spp, " / ".join("%.4f" % e for e in row["e_plain"]), " / ".join("%.4f" % e for e in row["e_unknown"]),
                                                  " / ".join("%.4f" % e for e in row["e_spatial"])))
    for name, t in sorted((chains or {}).items()):
        lines.append("%s chain, %d spp   frame   plain     temporal, off   temporal + estimate" % (name, CHAIN_SPP))
        lines += ["%s chain           %5d   %.4f    %.4f          %.4f" % (name, f, p, off, on) for f, (p, off, on) in enumerate(zip(t["e_plain"], t["e_off"], t["e_on"]), 1)]
    return "\n".join(lines)
