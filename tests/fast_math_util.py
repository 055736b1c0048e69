"""The comparison rule for HJR_FLAG_FAST_MATH frames and the reference frames it needs.

A fast-math frame is not bit-exact by contract, and a discrete decision (lobe choice, roulette, `xi < p`, a weight step of the 1.8
fixed-point texel filter) may fall the other way on a few samples.  The reference is the oracle's MATH_LIBM frame at the same sample
stream.  For each of colour, albedo and normal (.xyz):

  scale(p)      = max(max_c |ref_c(p)|, FLOOR)
  p disagrees   when max_c |got_c(p) - ref_c(p)| > tol * scale(p); a non-finite `got` always disagrees
  n_ref         = the larger of the counts of pixels in which the oracle's MATH_PORTABLE and MATH_HOSTF64 frames disagree with the LIBM
                  frame at TOL_REF: the pixels that hold a decision within an arithmetic's error of its threshold (the reference alone
                  supplies it)
  bar           n_bad <= max(2, ceil(0.005 * pixels)) + 4 * n_ref at TOL, every value finite, colour alpha 1

One frame of the suite has a reference that is not finite: the zero-length vertex normals of shading_cases.shading_normals make the
normal AOV NaN in 15 pixels, the same 15 in all three oracle modes and (bit for bit) on the exact kernels; normalize() of a zero vector
is 0 * inf in every arithmetic.  The colour frame is finite there (the sample guard).  In a pixel whose reference is not finite, `got`
agrees when it is not finite either and disagrees when it is finite, and "every value finite" is asked of the pixels whose reference
is finite.  The host test pins that no other frame and no other AOV has such pixels.

TOL is the project's tolerance figure (BASELINE.json north star), used relative here.  The additive part allows the handful of flips a
frame of about 1e5 decisions can hold at fast-math error sizes, the factor 4 is margin: fast math perturbs every division, root and
fused multiply-add, not only the transcendental calls in which the three CPU modes differ.  tests/test_fast_math_cases_host.py pins the
condition the cap rests on (n_ref <= 3 % of the pixels) on the CPU; tests/test_gpu_fast_math_cases.py holds the GPU frames to the bar."""
import math

import numpy as np

import oracle_binding as ob

TOL_REF = 1e-4      # n_ref: PORTABLE / HOSTF64 against LIBM
TOL = 1e-3          # the bar of a fast-math frame
FLOOR = 1e-3        # scale of a black pixel
ADD_FRACTION = 0.005
ADD_MIN = 2
REF_FACTOR = 4
N_REF_MAX_FRACTION = 0.03  # the condition of the cap (host test)
AOVS = ("color", "albedo", "normal")


def disagree(got, ref, tol):
    """bool [h, w]: the pixels of `got` that disagree with `ref` at `tol` (first three channels)"""
    g = np.asarray(got, dtype=np.float64)[..., :3]
    r = np.asarray(ref, dtype=np.float64)[..., :3]
    ref_ok, got_ok = np.isfinite(r).all(axis=-1), np.isfinite(g).all(axis=-1)
    with np.errstate(invalid="ignore"):
        scale = np.maximum(np.abs(r).max(axis=-1), FLOOR)
        d = np.abs(g - r).max(axis=-1)
        return np.where(ref_ok, ~(d <= tol * scale) | ~got_ok, got_ok)


def n_bad(got, ref, tol=TOL):
    return int(disagree(got, ref, tol).sum())


def cap(pixels, n_ref):
    return max(ADD_MIN, int(math.ceil(ADD_FRACTION * pixels))) + REF_FACTOR * n_ref


class Reference:
    """The LIBM frame of one scene and parameter set (colour, albedo, normal; read-only) and n_ref per AOV."""

    def __init__(self, arrays, params):
        frames = {}
        for mode in (ob.MATH_LIBM, ob.MATH_PORTABLE, ob.MATH_HOSTF64):
            osc = ob.OracleScene(arrays, mode)
            try:
                frames[mode] = osc.render(params)[:3]
            finally:
                osc.close()
        self.frames = dict(zip(AOVS, frames[ob.MATH_LIBM]))
        for a in self.frames.values():
            a.setflags(write=False)
        self.pixels = params.width * params.height
        self.n_ref_by_mode = {aov: tuple(n_bad(frames[m][i], frames[ob.MATH_LIBM][i], TOL_REF) for m in (ob.MATH_PORTABLE, ob.MATH_HOSTF64))
                              for i, aov in enumerate(AOVS)}
        self.n_ref = {aov: max(v) for aov, v in self.n_ref_by_mode.items()}

    def cap(self, aov):
        return cap(self.pixels, self.n_ref[aov])

    def check(self, got, what):
        """Holds the frames {aov: array or None} of a fast-math launch to the bar; prints n_bad next to its cap for every AOV given."""
        fails = []
        for aov in AOVS:
            g = got.get(aov)
            if g is None:
                continue
            n, c = n_bad(g, self.frames[aov]), self.cap(aov)
            print("fast-math %s %s: n_bad %d, cap %d (n_ref %d, %d pixels)" % (what, aov, n, c, self.n_ref[aov], self.pixels))
            if not np.isfinite(np.asarray(g)[np.isfinite(self.frames[aov]).all(axis=-1)]).all():
                fails.append("%s holds non-finite values where the reference is finite" % aov)
            if n > c:
                bad = np.argwhere(disagree(g, self.frames[aov], TOL))
                y, x = bad[0]
                fails.append("%s: n_bad %d > cap %d; first at (x=%d, y=%d): fast %s, LIBM oracle %s"
                             % (aov, n, c, x, y, np.asarray(g)[y, x, :3], self.frames[aov][y, x, :3]))
        if got.get("color") is not None and not (np.asarray(got["color"])[..., 3] == 1).all():
            fails.append("colour alpha is not 1 everywhere")
        assert not fails, "%s: %s" % (what, "; ".join(fails))


# ------------------------------------------------------------------ the frames of the two test files, by key, computed once
TABLE_W, TABLE_H, TABLE_SPP = 72, 48, 5            # tests/test_gpu_scene_tables.py
TABLE_SCENES = ("lights171", "lights200", "mats205", "mats210", "textured", "textured_no_mr")
CHUNK_W, CHUNK_H, CHUNK_SPP = 21, 13, 32            # the smallest shape of tests/test_gpu_item_chunks.py: 4 chunks of 8, a ragged frame
TEX_CHUNK_SPP = 16                                  # the textured scene with two chunks per pixel (A = 2 kernels, items of two chunks)
INTEGRATORS = {"nee": ob.INTEGRATOR_NEE, "pt": ob.INTEGRATOR_PT}

_refs = {}
_cornell = None


def cornell():
    global _cornell
    if _cornell is None:
        from scene_util import Cornell
        _cornell = Cornell()
    return _cornell


def case_reference(name, iname):
    """a case of shading_cases.cases() at its own size"""
    k = ("case", name, iname)
    if k not in _refs:
        import shading_cases as sc
        c = sc.cases()[name]
        _refs[k] = Reference(c.oracle_arrays(), c.oracle_params(sc.INTEGRATORS[iname]))
    return _refs[k]


def table_reference(name, iname, spp=TABLE_SPP):
    """a scene of table_util at 72 x 48"""
    k = ("table", name, iname, spp)
    if k not in _refs:
        import table_util as tu
        s = tu.scene(name)
        _refs[k] = Reference(s.arrays, s.oracle_params(TABLE_W, TABLE_H, spp, integrator=INTEGRATORS[iname]))
    return _refs[k]


def chunk_reference(iname):
    """the bundled Cornell box at the item-chunk shape"""
    k = ("chunks", iname)
    if k not in _refs:
        s = cornell()
        _refs[k] = Reference(s.arrays, s.oracle_params(CHUNK_W, CHUNK_H, CHUNK_SPP, integrator=INTEGRATORS[iname]))
    return _refs[k]
