"""Shared by the coverage tests of the temporal accumulation (hjr_render_gbuffer_cov, hjr_temporal_frame.coverage, option
"denoise_temporal_coverage"): the native checker tests/native/temporal_cov_ref.cpp (built once per process with g++ -O2
-ffp-contract=off; it restates the header comment of csrc/hjr_temporal.hip.h: a brute-force coverage pass and the accumulation with rules
2' and 3'), the inputs it takes, and the cameras and sequences the GPU tests, tools/temporal_rehearsal.py and tools/temporal_bench.py use."""
import os
import subprocess

import numpy as np

import trace_util
from scene_util import hjr
from temporal_util import _side_bytes, build_checker, cam_floats, camera_at, moved_consistent, ref_mask, rmse

f32 = np.float32
SNAP = f32(0.125)

def pad_word(same, total):
    return np.uint32(same | (total << 8))


def mixed(gbuffer):
    """The mixed rule on the pad words of a G-buffer of a side with coverage: total > 0 and same < total."""
    pad = np.asarray(gbuffer["pad"], np.uint32)
    total = (pad >> 8) & 0xff
    return (total > 0) & ((pad & 0xff) < total)


# ---- the coverage pass
def rows_from_arrays(arrays):
    """Triangle rows of the checker from the scene arrays alone (no GPU): [n, 12] float32 (v0, v1, v2, prim id bits, 0, 0), tri_inst and
    material ids.  The vertices are trace_util.world_triangles': the builders' bits for translations, within an ulp otherwise."""
    tris = trace_util.world_triangles(arrays)
    n = tris.shape[0]
    rows = np.zeros((n, 12), f32)
    rows[:, :9] = tris.reshape(n, 9)
    rows[:, 9] = np.arange(n, dtype=np.uint32).view(f32)
    po = np.asarray(arrays["prim_offsets"]).reshape(-1)
    inst = (np.searchsorted(po, np.arange(n), side="right") - 1).astype(np.uint32)
    return rows, inst, np.asarray(arrays["material_ids"], np.uint32).reshape(-1).copy()


def rows_from_device(dev, arrays):
    """The same from the frame data the device holds (either builder): the leaf-ordered triangle array as it is, instance ids from the
    scene's prim offsets, material ids from the scene arrays (the kernel reads them from word 15 of the shading rows: checked apart)."""
    rows = dev.copy_frame_data(hjr.FRAME_TRI_GEOM).reshape(-1, 12).copy()
    n = np.asarray(arrays["indices"]).size // 3
    po = np.asarray(arrays["prim_offsets"]).reshape(-1)
    inst = (np.searchsorted(po, np.arange(n), side="right") - 1).astype(np.uint32)
    return rows, inst, np.asarray(arrays["material_ids"], np.uint32).reshape(-1).copy()


def gbuffer_cov_ref(rows, tri_inst, tri_mat, w, h, cam, side):
    """The native checker's coverage pass (side 0: the plain G-buffer): GBUFFER_DTYPE [h, w]."""
    exe, tmp = build_checker("temporal_cov_ref")
    src, dst = os.path.join(tmp, "g_in.bin"), os.path.join(tmp, "g_out.bin")
    rows = np.ascontiguousarray(rows, f32).reshape(-1, 12)
    with open(src, "wb") as f:
        f.write(cam_floats(cam).tobytes() + rows.tobytes() + np.ascontiguousarray(tri_inst, np.uint32).tobytes() + np.ascontiguousarray(tri_mat, np.uint32).tobytes())
    subprocess.check_call([exe, "gbuf", str(w), str(h), str(side), str(rows.shape[0]), str(len(tri_inst)), src, dst])
    return np.fromfile(dst, hjr.GBUFFER_DTYPE).reshape(h, w)


# ---- the accumulation
def temporal_cov_ref(prev, cur, n_tris, snap=None):
    """The native checker's accumulation on dicts as Device.temporal_accumulate takes them (key "coverage" per side, absent = 0):
    (color [h, w, 4], variance [h, w], history [h, w])."""
    exe, tmp = build_checker("temporal_cov_ref")
    h, w = np.asarray(cur["gbuffer"]).shape
    n_inst = np.asarray(cur["transforms"], f32).size // 12
    src, dst = os.path.join(tmp, "a_in.bin"), os.path.join(tmp, "a_out.bin")
    with open(src, "wb") as f:
        if prev is not None:
            f.write(_side_bytes(prev, True))
        f.write(_side_bytes(cur, False))
    cmd = [exe, "acc", str(w), str(h), str(n_inst), str(int(n_tris)), "1" if prev is not None else "0",
           str(int((prev or {}).get("coverage") or 0)), str(int(cur.get("coverage") or 0)), src, dst]
    if snap is not None:
        cmd.append(repr(float(snap)))
    subprocess.check_call(cmd)
    raw = np.fromfile(dst, f32)
    assert raw.size == w * h * 6
    return raw[:w * h * 4].reshape(h, w, 4), raw[w * h * 4:w * h * 5].reshape(h, w), raw[w * h * 5:].reshape(h, w)


# ---- cameras
def wall_view(cornell):
    """Test (b)'s view: inside the box, so close to one wall that the wall fills the frame."""
    return camera_at(cornell, x=-0.9)


def reprojection(prev, cur):
    """float64 restatement of step 2 for diagnostics: (xp, yp) [h, w] of the current frame's hit pixels in the previous frame (NaN for
    misses).  Not bit-exact; tests use it only well away from a threshold."""
    g = cur["gbuffer"]
    h, w = g.shape
    hit = g["prim"] != 0xffffffff
    inst = np.where(hit, g["inst"], 0).astype(np.int64)
    inv = np.asarray(cur["inv_transforms"], np.float64).reshape(-1, 3, 4)[inst]
    m = np.asarray(prev["transforms"], np.float64).reshape(-1, 3, 4)[inst]
    p = g["pos"].astype(np.float64)
    po = np.einsum("hwij,hwj->hwi", inv[..., :3], p) + inv[..., 3]
    pp = np.einsum("hwij,hwj->hwi", m[..., :3], po) + m[..., 3]
    c = cam_floats(prev["camera"]).astype(np.float64)
    a, up, right = c[3:6] * c[12], c[6:9], c[9:12]
    sol = np.linalg.solve(np.stack([a, right, up], axis=1), (pp - c[0:3]).reshape(-1, 3).T).T.reshape(h, w, 3)
    u, v = sol[..., 1] / sol[..., 0], sol[..., 2] / sol[..., 0]
    xp, yp = (u * h + w) * 0.5 - 0.5, (v * h + h) * 0.5 - 0.5
    return np.where(hit, xp, np.nan), np.where(hit, yp, np.nan)


# ---- the quality comparison (§11.5): §11.2's set-up with a third column, the temporal path with coverage
def quality_table_cov(refs, out_var, out_tmp, out_cov):
    masks = [ref_mask(r) for r in refs]
    t = {"mask_share": [float(m.mean()) for m in masks]}
    for key, outs in (("var", out_var), ("tmp", out_tmp), ("cov", out_cov)):
        t["e_" + key] = [rmse(o, r, m) for o, r, m in zip(outs, refs, masks)]
        d = [float(np.abs(outs[f][..., :3].astype(np.float64) - outs[f - 1][..., :3])[masks[f] & masks[f - 1]].mean()) for f in range(4, len(outs))]
        t["flicker_" + key] = float(np.mean(d))
    return t


def conditions_s(t):
    """§11.2's four conditions on the static sequence with e_cov in place of e_tmp."""
    ev, ec = t["e_var"], t["e_cov"]
    return [("e_cov(8) %.5f < e_var(8) %.5f" % (ec[7], ev[7]), ec[7] < ev[7]),
            ("mean e_cov(4..8) %.5f < mean e_var(4..8) %.5f" % (np.mean(ec[3:8]), np.mean(ev[3:8])), np.mean(ec[3:8]) < np.mean(ev[3:8])),
            ("e_cov(8) %.5f < e_cov(2) %.5f" % (ec[7], ec[1]), ec[7] < ec[1]),
            ("flicker_cov %.5f < flicker_var %.5f" % (t["flicker_cov"], t["flicker_var"]), t["flicker_cov"] < t["flicker_var"])]


def conditions_m(t):
    """The two claims on the moving sequence."""
    et, ec = t["e_tmp"], t["e_cov"]
    return [("mean e_cov(4..8) %.5f < mean e_tmp(4..8) %.5f" % (np.mean(ec[3:8]), np.mean(et[3:8])), np.mean(ec[3:8]) < np.mean(et[3:8])),
            ("e_cov(3) %.5f < e_tmp(3) %.5f" % (ec[2], et[2]), ec[2] < et[2])]


def format_table_cov(name, t):
    lines = ["%s   frame   e_var     e_tmp     e_cov" % name]
    lines += ["%s   %5d   %.5f   %.5f   %.5f" % (name, f + 1, a, b, c) for f, (a, b, c) in enumerate(zip(t["e_var"], t["e_tmp"], t["e_cov"]))]
    lines.append("%s   flicker (f = 5..8): per-frame filter %.5f, temporal %.5f, temporal with coverage %.5f" % (name, t["flicker_var"], t["flicker_tmp"], t["flicker_cov"]))
    return "\n".join(lines)


def quality_sequences_cov(cornell, dev, side, w=96, h=64, spp=16, frames=8, ref_spp=4096, seed=1):
    """temporal_util.quality_sequences with the coverage column: the same renders feed the per-frame filter, the temporal path with the
    plain G-buffer and the temporal path with the coverage G-buffer of `side`."""
    cam = camera_at(cornell, x=3.5)
    kw = dict(sky=tuple(cornell.opt.scene_sky_default), ibl_intensity=cornell.opt.IBL_intensity)
    tables = {}
    for name, static in (("S", True), ("M", False)):
        refs, outs, prev = [], {"var": [], "tmp": [], "cov": []}, {"tmp": None, "cov": None}
        for f in range(1, frames + 1):
            xf = moved_consistent(cornell.arrays, 0 if static else f)
            dev.set_transforms(*xf)
            if f == 1 or not static:
                ref = dev.render(hjr.make_params(w, h, ref_spp, cam, seed=7, **kw), want_aovs=False)[0]
            refs.append(ref)
            p = hjr.make_params(w, h, spp, cam, frame=f, seed=seed, **kw)
            c, a, n, v = dev.render(p, want_variance=True)
            outs["var"].append(dev.denoise(hjr.MODE_DENOISE, c, a, n, variance=v))
            for key, cov in (("tmp", 0), ("cov", side)):
                cur = {"camera": cam, "transforms": xf[0], "inv_transforms": xf[1], "gbuffer": dev.gbuffer(p, coverage=cov), "color": c, "variance": v, "coverage": cov}
                tc, tv, th = dev.temporal_accumulate(prev[key], cur)
                outs[key].append(dev.denoise(hjr.MODE_DENOISE, tc, a, n, variance=tv))
                prev[key] = dict(cur, color=tc, variance=tv, history=th)
        tables[name] = quality_table_cov(refs, outs["var"], outs["tmp"], outs["cov"])
    return tables
