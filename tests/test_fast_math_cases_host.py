"""The condition the fast-math comparison rule rests on (tests/fast_math_util.py), pinned on the CPU: in every frame
tests/test_gpu_fast_math_cases.py renders, the oracle's own three arithmetics (MATH_LIBM against MATH_PORTABLE and MATH_HOSTF64) disagree
in at most 3 % of the pixels at 1e-4 (measured maximum 2.9 %: grazing_lens under NEE, 30 of 1024 pixels), and the LIBM frame, the
reference of the GPU test, is finite, but for the 15 pixels of one normal AOV named in NOT_FINITE, on which the three arithmetics agree.
The helper itself is checked on synthetic arrays."""
import numpy as np
import pytest

import fast_math_util as fm
import shading_cases as sc


# the one reference that is not finite (fast_math_util): the patch of zero-length vertex normals, normal AOV only.  n_ref counts a pixel
# in which one oracle mode is finite and another is not, so n_ref == 0 there says that the three modes agree on these pixels.
NOT_FINITE = {("shading_normals", "normal"): 15}


def check_reference(ref, what):
    for aov in fm.AOVS:
        holes = int((~np.isfinite(ref.frames[aov]).all(axis=-1)).sum())
        assert holes == NOT_FINITE.get((what.split()[0], aov), 0), "%s: the LIBM %s frame is not finite in %d pixels" % (what, aov, holes)
        assert not holes or ref.n_ref[aov] == 0  # PORTABLE and HOSTF64 are not finite in exactly those pixels, and equal LIBM elsewhere
        print("%s %s: %d pixels, PORTABLE / HOSTF64 count at 1e-4: %d / %d" % ((what, aov, ref.pixels) + ref.n_ref_by_mode[aov]))
        assert ref.n_ref[aov] <= fm.N_REF_MAX_FRACTION * ref.pixels, (what, aov, ref.n_ref[aov], ref.pixels)
        assert ref.cap(aov) == max(2, -(-ref.pixels // 200)) + 4 * ref.n_ref[aov]
    assert (ref.frames["color"][..., 3] == 1).all(), what


@pytest.mark.parametrize("iname", list(fm.INTEGRATORS))
@pytest.mark.parametrize("name", list(sc.cases()))
def test_shading_case_reference(name, iname):
    c = sc.cases()[name]
    ref = fm.case_reference(name, iname)
    assert ref.pixels == c.w * c.h
    check_reference(ref, "%s %s" % (name, iname))


@pytest.mark.parametrize("iname", list(fm.INTEGRATORS))
@pytest.mark.parametrize("name", fm.TABLE_SCENES)
def test_table_scene_reference(name, iname):
    ref = fm.table_reference(name, iname)
    assert ref.pixels == fm.TABLE_W * fm.TABLE_H
    check_reference(ref, "%s %s" % (name, iname))


@pytest.mark.parametrize("iname", list(fm.INTEGRATORS))
def test_item_chunk_references(iname):
    check_reference(fm.chunk_reference(iname), "bundled scene %dx%dx%d %s" % (fm.CHUNK_W, fm.CHUNK_H, fm.CHUNK_SPP, iname))
    check_reference(fm.table_reference("textured", iname, fm.TEX_CHUNK_SPP), "textured at %d spp %s" % (fm.TEX_CHUNK_SPP, iname))


# ------------------------------------------------------------------ the helper on synthetic arrays
def frame(h=6, w=5):
    rng = np.random.default_rng(3)
    f = np.ones((h, w, 4), np.float32)
    f[..., :3] = rng.uniform(0.05, 4.0, (h, w, 3)).astype(np.float32)
    return f


def test_equal_frames_agree():
    f = frame()
    assert fm.n_bad(f, f) == 0 and fm.n_bad(f, f, fm.TOL_REF) == 0
    z = np.zeros((4, 4, 4), np.float32)
    assert fm.n_bad(z, z) == 0


def test_one_nan_pixel_counts_as_one():
    f = frame()
    for v in (np.nan, np.inf, -np.inf):
        g = f.copy()
        g[2, 3, 1] = v
        assert fm.n_bad(g, f) == 1 and fm.disagree(g, f, fm.TOL)[2, 3]
    g = f.copy()
    g[1, 1, :3] = np.nan
    g[1, 2, 0] = np.nan
    assert fm.n_bad(g, f) == 2


def test_pixel_whose_reference_is_not_finite():
    f = frame()
    f[2, 2, :3] = np.nan
    g = f.copy()
    assert fm.n_bad(g, f) == 0          # NaN where the reference is NaN
    g[2, 2, :3] = 0.5
    assert fm.n_bad(g, f) == 1          # finite where the reference is not
    g[2, 2, :3] = (0.5, np.inf, 0.5)
    assert fm.n_bad(g, f) == 0


def test_relative_threshold():
    f = frame()
    scale = np.abs(f[..., :3]).max(axis=-1)
    g = f.copy()
    g[0, 0, 2] += np.float32(2e-3 * scale[0, 0])   # counts
    g[3, 4, 0] -= np.float32(5e-4 * scale[3, 4])   # does not
    bad = fm.disagree(g, f, fm.TOL)
    assert bad[0, 0] and not bad[3, 4] and bad.sum() == 1
    # the scale is the pixel's largest reference channel, not the channel's own value
    f[5, 0, :3] = (4.0, 0.01, 0.01)
    g = f.copy()
    g[5, 0, 1] += np.float32(2e-3)                 # 20 % of its channel, 5e-4 of the pixel's scale
    assert fm.n_bad(g, f) == 0
    g[5, 0, 1] += np.float32(8e-3)                 # 2.5e-3 of the scale
    assert fm.n_bad(g, f) == 1
    # alpha takes no part
    g = f.copy()
    g[..., 3] = 0.5
    assert fm.n_bad(g, f) == 0


def test_floor_applies_to_a_black_pixel():
    ref = np.zeros((2, 2, 4), np.float32)
    got = ref.copy()
    got[0, 0, 0] = 5e-7   # below TOL * FLOOR = 1e-6
    got[1, 1, 2] = 2e-6   # above it
    bad = fm.disagree(got, ref, fm.TOL)
    assert not bad[0, 0] and bad[1, 1] and bad.sum() == 1
    ref[0, 1, :3] = 5e-4  # a reference below the floor: the floor is still the scale
    got = ref.copy()
    got[0, 1, 1] += np.float32(8e-7)
    assert fm.n_bad(got, ref) == 0


def test_cap():
    assert fm.cap(64, 0) == 2 and fm.cap(1024, 0) == 6 and fm.cap(1024, 30) == 126 and fm.cap(72 * 48, 1) == 18 + 4
    assert fm.cap(401, 0) == 3  # ceil, not round
