"""The wave-uniform control flow of the LDS-resident traversal pass (hjr_traverse.hip.h: ray_tri<true>'s exits on a ballot, the leaf loop's
one "some lane hit" branch with the closest-hit update as selects, the shadow lane that leaves the loop by zeroing its count) decides per
WAVE what used to be decided per lane.  What it can get wrong are waves whose lanes disagree, so the batches here are built by hand, wave
by wave of 64 pairs, over a scene of eight clusters of four triangles (one cluster is one leaf when leaf_max is 4):

  stage waves   one lane reaching each stage of the triangle test (rejected at u, at v, at t, or hitting) while the other 63 are rejected at
                each earlier stage (det, u, v, t), and the reverse: 63 lanes deep in the test, one rejected early
  degenerate    lanes that hit beside lanes whose leaf holds a triangle with two equal vertices (det == 0 for every ray)
  leaf order    shadow-only lanes occluded by each triangle of a cluster beside closest-only lanes that hit each other triangle: with the
                cluster in one leaf, one shadow lane leaves at the leaf's first triangle while a closest lane hits only its last;
                lanes that carry both rays start their closest-hit ray while the neighbours are in the middle of the leaf
  equal t       exact duplicates of two triangles: the smaller prim id wins, whichever the leaf holds first
  unlike lanes  shadow rays that leave the scene at once, that are occluded, and that graze four triangles in their plane, each with a
                closest-hit ray into another cluster
  non-finite    NaN / infinite origins and directions in every eighth lane of a leaf-order wave
  partial waves the first 1, 63 and 65 pairs

The reference is the oracle's brute force over all triangles (tests/trace_util.py); every batch is first checked against it on the CPU
(each lane does what the wave was built for), then hjr_trace_rays must return the reference bit for bit on both traversal loops and the
default, stack16, leaf4, node_min1 and node_min64 configurations.  A counting render of the Cornell box must give the same ten counters
with node_min 1 as with the default: the descent loop's test reads `n_inner < node_min` alone."""
import numpy as np
import pytest

import oracle_binding as ob
import trace_util as tu
from scene_util import Cornell, hjr, new_device

pytestmark = pytest.mark.gpu

F32 = np.float32
PATHS = {"standalone": hjr.TRACE_STANDALONE, "fused": hjr.TRACE_FUSED}
CONFIGS = {
    "default": {},
    "stack16": dict(lds_stack16=1),
    "leaf4": dict(leaf_max=4),
    "node_min1": dict(node_min=1),
    "node_min64": dict(node_min=64),
}
N_CLUSTERS, DEGENERATE, EQUAL_T = 8, 5, 6  # cluster c holds prims 4c .. 4c + 3
E, H = 0.375, 0.25  # edge length and rise of a triangle: (x0, y0, 0) (x0 + E, y0, 0) (x0, y0 + E, H), x0 = k / 2, y0 = 8 c
DET, U, V, T, HIT = range(5)  # where the canonical test leaves a ray


def cluster_triangles():
    t = np.zeros((N_CLUSTERS, 4, 3, 3), F32)
    for c in range(N_CLUSTERS):
        for k in range(4):
            x0, y0 = 0.5 * k, 8.0 * c
            t[c, k] = [[x0, y0, 0], [x0 + E, y0, 0], [x0, y0 + E, H]]
    t[DEGENERATE, 3, 1] = t[DEGENERATE, 3, 0]  # two equal vertices: e1 == 0, det == 0 for every ray
    t[EQUAL_T, 2], t[EQUAL_T, 3] = t[EQUAL_T, 0], t[EQUAL_T, 1]  # prims 26, 27 duplicate prims 24, 25
    return t.reshape(-1, 3, 3)


def scene_arrays():
    t = cluster_triangles()
    n = t.shape[0]
    mats = np.zeros(1, hjr.MATERIAL_DTYPE)
    mats[0]["basecolor"] = (0.5, 0.5, 0.5)
    mats[0]["roughness"] = 0.5
    mats[0]["ior"] = 1.0
    for k in ("basecolor_tex", "metallic_roughness_tex", "normal_tex", "emission_tex"):
        mats[0][k] = -1
    return dict(vertices=t.reshape(-1, 3), normals=np.tile(np.array([[0, 0, 1]], F32), (3 * n, 1)), texcoords=np.zeros((3 * n, 2), F32),
                indices=np.arange(3 * n, dtype=np.uint32), material_ids=np.zeros(n, np.uint32), prim_offsets=np.zeros(1, np.uint32),
                transforms=tu.IDENTITY.copy(), inv_transforms=tu.IDENTITY.copy(), materials=mats, light_prim_ids=np.zeros(0, np.uint32),
                light_prim_emission=np.zeros(0, F32))


def stage_of(tri, o, d, tmax):
    """where ray_tri leaves the ray: the stages of the canonical test in float32 (no fused multiply-add: the rays keep clear of every
    boundary but det == 0, whose products are exact zeros)"""
    v0, v1, v2 = tri.astype(F32)
    o, d = np.asarray(o, F32), np.asarray(d, F32)
    e1, e2 = v1 - v0, v2 - v0
    p = np.cross(d, e2).astype(F32)
    det = F32(np.dot(e1, p))
    if det == 0:
        return DET
    tv = o - v0
    u = F32(np.dot(tv, p)) / det
    if not (0 <= u <= 1):
        return U
    q = np.cross(tv, e1).astype(F32)
    v = F32(np.dot(d, q)) / det
    if not (v >= 0 and u + v <= 1):
        return V
    t = F32(np.dot(e2, q)) / det
    return HIT if tu.TMIN < t < tmax else T


DOWN = (0.0, 0.0, -1.0)


def ray_of(kind, c, k):
    """(origin, direction, tmax as a shadow ray) of a ray that the test of triangle k of cluster c leaves at `kind`"""
    x0, y0 = 0.5 * k, 8.0 * c
    if kind == DET:  # along x in the triangles' plane z = 2/3 (y - y0): crosses the boxes of all four, det == 0 for each
        return (-1.0, y0 + 0.125, 0.0625), (1.0, 0.0, 0.0), 8.0
    if kind == U:  # the gap between triangle k and the next: inside the cluster's box, outside [0, 1] in u for all four
        return (x0 + 0.4375, y0 + 0.125, 1.0), DOWN, 8.0
    if kind == V:  # inside the triangle's box, beyond its hypotenuse: u = v = 2/3
        return (x0 + 0.25, y0 + 0.25, 1.0), DOWN, 8.0
    if kind == T:  # over the triangle (hit at t = 11/12), as a shadow ray that ends inside its box (entered at t = 0.75)
        return (x0 + 0.125, y0 + 0.125, 1.0), DOWN, 0.85
    return (x0 + 0.125, y0 + 0.125, 1.0), DOWN, 8.0


AWAY = ((0.25, 0.25, 2.0), (0.0, 0.0, 1.0), 8.0)  # leaves the scene at once


class Wave:
    """64 pairs: per lane the shadow ray, the closest-hit ray (None: not valid) and what the lane must come to"""

    def __init__(self, name):
        self.name, self.sh, self.cl, self.want = name, [], [], []

    def lane(self, sh=None, cl=None, occluded=None, prim=None):
        self.sh.append(sh); self.cl.append(cl); self.want.append((occluded, prim))

    def rays(self):
        assert len(self.sh) == 64, self.name

        def pack(rs, closest):
            r = np.zeros(64, hjr.RAY_DTYPE)
            for i, x in enumerate(rs):
                o, d, tmax = x if x is not None else AWAY
                r["o"][i], r["d"][i] = o, d
                r["tmax"][i] = F32(1e16) if closest else F32(tmax)
                r["valid"][i] = 0 if x is None else 1
            return r
        return pack(self.sh, False), pack(self.cl, True)


def stage_waves():
    """(deep kind, shallow kind), one lane against 63 and 63 against one, the ray in the shadow slot and in the closest-hit slot (no
    closest-hit ray fails at t: its far end is 1e16)"""
    waves = []
    for slot, kinds in (("shadow", (DET, U, V, T, HIT)), ("closest", (DET, U, V, HIT))):
        for deep in kinds[1:]:
            for shallow in [x for x in kinds if x < deep]:
                for single in (deep, shallow):
                    rest = shallow if single == deep else deep
                    n = len(waves)
                    c, k, at = n % 5, n % 4, (7 * deep + 13 * shallow + 29 * (single == deep)) % 64
                    w = Wave("%s slot: one lane at stage %d, 63 at stage %d, cluster %d triangle %d" % (slot, single, rest, c, k))
                    for lane in range(64):
                        kind = single if lane == at else rest
                        r = ray_of(kind, c, k)
                        hit = kind == HIT
                        if slot == "shadow":
                            w.lane(sh=r, occluded=int(hit))
                        else:
                            w.lane(cl=r, occluded=0, prim=4 * c + k if hit else tu.NO_PRIM)
                    w.kinds = (single, rest, at, c, k, slot)
                    waves.append(w)
    return waves


def degenerate_wave():
    w = Wave("degenerate triangle beside lanes that hit")
    c = DEGENERATE
    over = ((1.5, 8.0 * c + 0.125, 1.0), DOWN, 8.0)  # over the degenerate triangle's segment x = 1.5
    for lane in range(64):
        k = lane % 4
        if k == 3:
            w.lane(sh=over, cl=over, occluded=0, prim=tu.NO_PRIM)
        elif lane % 8 < 4:
            w.lane(cl=ray_of(HIT, c, k), occluded=0, prim=4 * c + k)
        else:
            w.lane(sh=ray_of(HIT, c, k), cl=ray_of(HIT, c, (k + 1) % 3), occluded=1, prim=4 * c + (k + 1) % 3)
    return w


def leaf_order_wave(c):
    w = Wave("leaf order, cluster %d" % c)
    for lane in range(64):
        i, j = (lane // 3) % 4, (lane // 12) % 4
        if lane % 3 == 0:
            w.lane(sh=ray_of(HIT, c, i), occluded=1, prim=tu.NO_PRIM)
        elif lane % 3 == 1:
            w.lane(cl=ray_of(HIT, c, i), occluded=0, prim=4 * c + i)
        else:
            w.lane(sh=ray_of(HIT, c, i), cl=ray_of(HIT, c, j), occluded=1, prim=4 * c + j)
    return w


def equal_t_wave():
    w = Wave("equal t: the smaller prim id wins")
    c = EQUAL_T
    for lane in range(64):
        k = lane % 2  # triangles 0 and 1; 2 and 3 are their duplicates, at the same place
        if lane % 4 < 2:
            w.lane(cl=ray_of(HIT, c, k), occluded=0, prim=4 * c + k)
        else:
            w.lane(sh=ray_of(HIT, c, k), cl=ray_of(HIT, c, 1 - k), occluded=1, prim=4 * c + (1 - k))
    return w


def unlike_wave():
    w = Wave("unlike lanes")
    for lane in range(64):
        c, k = lane % 5, lane % 4
        cc, kk = (lane * 3 + 1) % 5, (lane + 1) % 4
        cl = ray_of(HIT, cc, kk)
        m = lane % 4
        if m == 0:
            w.lane(sh=AWAY, cl=cl, occluded=0, prim=4 * cc + kk)
        elif m == 1:
            w.lane(sh=ray_of(HIT, c, k), cl=cl, occluded=1, prim=4 * cc + kk)
        elif m == 2:
            w.lane(sh=ray_of(DET, c, k), cl=cl, occluded=0, prim=4 * cc + kk)
        else:
            w.lane(sh=ray_of(T, c, k), cl=ray_of(V, cc, kk), occluded=0, prim=tu.NO_PRIM)
    return w


class Batch:
    def __init__(self):
        self.arrays = scene_arrays()
        self.tris = cluster_triangles()
        self.osc = ob.OracleScene(self.arrays, ob.MATH_PORTABLE)
        self.waves = stage_waves() + [degenerate_wave(), leaf_order_wave(0), leaf_order_wave(7), equal_t_wave(), unlike_wave()]
        parts = [w.rays() for w in self.waves]
        # non-finite rays beside finite ones: a leaf-order wave with every eighth lane spoiled (no expectation but the brute force's)
        sh, cl = leaf_order_wave(3).rays()
        bad = np.array([np.nan, np.inf, -np.inf], F32)
        for i, lane in enumerate(range(3, 64, 8)):
            (sh if i % 2 else cl)["od"[(i // 2) % 2]][lane, i % 3] = bad[i % 3]
        self.n_checked = 64 * len(parts)
        parts.append((sh, cl))
        self.shadow = np.concatenate([p[0] for p in parts])
        self.closest = np.concatenate([p[1] for p in parts])
        self.ref = tu.brute_reference(self.osc, self.shadow, self.closest)
        self.check_on_cpu()

    def check_on_cpu(self):
        """the reference alone: every lane does what its wave was built for"""
        want = [x for w in self.waves for x in w.want]
        for i, (occluded, prim) in enumerate(want):
            w = self.waves[i // 64]
            if occluded is not None:
                assert self.ref["occluded"][i] == occluded, (w.name, i % 64, self.ref[i])
            if prim is not None:
                assert self.ref["prim"][i] == prim, (w.name, i % 64, self.ref[i])
        for w in self.waves:
            if hasattr(w, "kinds"):
                single, rest, at, c, k, slot = w.kinds
                rays = w.sh if slot == "shadow" else w.cl
                for lane in (at, (at + 1) % 64):
                    o, d, tmax = rays[lane]
                    assert stage_of(self.tris[4 * c + k], o, d, tmax if slot == "shadow" else 1e16) == (single if lane == at else rest), (w.name, lane)
        over = ((1.5, 8.0 * DEGENERATE + 0.125, 1.0), DOWN)
        assert stage_of(self.tris[4 * DEGENERATE + 3], over[0], over[1], 8.0) == DET
        # the equal-t lanes do meet two hits at one t: the duplicate alone gives the same t, b1, b2
        o, d, _ = ray_of(HIT, EQUAL_T, 0)
        assert stage_of(self.tris[4 * EQUAL_T + 2], o, d, 1e16) == HIT and np.array_equal(self.tris[4 * EQUAL_T], self.tris[4 * EQUAL_T + 2])
        assert np.isfinite(self.ref["t"]).all()


_batch = []


def batch():
    if not _batch:
        _batch.append(Batch())
    return _batch[0]


def check(dev, path, shadow, closest, ref, what):
    got = dev.trace_rays(path, shadow, closest)
    assert (got["status"] == hjr.TRACE_STATUS_OK).all(), (what, np.unique(got["status"], return_counts=True))
    bad = tu.mismatches(got, ref)
    if bad.size:
        b = batch()
        rows = [(b.waves[i // 64].name if i < b.n_checked else "non-finite wave", int(i % 64), got[i], ref[i]) for i in bad[:8]]
        pytest.fail("%s: %d of %d pairs differ from the brute force; first: %s" % (what, bad.size, got.size, rows))


@pytest.mark.parametrize("path_name", list(PATHS))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_waves_of_unlike_lanes(config, path_name):
    b = batch()
    dev = new_device(CONFIGS[config])
    try:
        dev.upload_arrays(b.arrays)
        dev.set_transforms(b.arrays["transforms"], b.arrays["inv_transforms"])
        check(dev, PATHS[path_name], b.shadow, b.closest, b.ref, "whole batch")
        st = dev.stats()
        print("%s %s: lds_mode %d, %d pairs" % (config, path_name, st["lds_mode"], b.shadow.size))
        assert st["lds_mode"] == (2 if config == "stack16" else 1), st["lds_mode"]  # the LDS-resident kernels are the ones under test
        if config == "leaf4":  # a cluster is one leaf: its four triangles lie side by side in the triangle table
            rows = dev.copy_frame_data(hjr.FRAME_TRI_GEOM).view(np.uint32).reshape(-1, 12)[:, 9]
            for c in range(N_CLUSTERS):
                at = np.flatnonzero((rows >= 4 * c) & (rows < 4 * c + 4))
                assert at.size == 4 and at.max() - at.min() == 3 and at.min() % 4 == 0, (c, at)
        first = 64 * (len(b.waves) - 4)  # the leaf-order wave of cluster 0 and what follows it
        for n in (1, 63, 65):
            check(dev, PATHS[path_name], b.shadow[:n], b.closest[:n], b.ref[:n], "first %d pairs" % n)
            check(dev, PATHS[path_name], b.shadow[first:first + n], b.closest[first:first + n], b.ref[first:first + n], "%d pairs from the leaf-order wave" % n)
    finally:
        dev.close()


COUNTERS = ("samples", "closest_rays", "shadow_rays", "box_tests_closest", "tri_tests_closest", "box_tests_shadow", "tri_tests_shadow",
            "shaded_hits", "light_samples", "nan_samples")


def test_counters_do_not_depend_on_node_min():
    """which boxes and triangles a ray tests is the tree's and the ray's business: a counting render of the Cornell box at 32 x 24, 16 spp
    counts the same with the descent loop's threshold at 1 (every pass goes on until no lane holds an inner node) as with the default"""
    cornell = Cornell()
    got = {}
    for name, options in (("default", {}), ("node_min1", dict(node_min=1))):
        d = cornell.device(options)
        try:
            d.render(cornell.hjr_params(32, 24, 16, integrator=hjr.INTEGRATOR_NEE, flags=hjr.FLAG_STATS), want_aovs=False)
            st = d.stats()
            assert st["lds_mode"] == 1, st["lds_mode"]
            got[name] = {k: int(st[k]) for k in COUNTERS}
        finally:
            d.close()
    print(got)
    assert got["default"]["samples"] == 32 * 24 * 16 and got["default"]["tri_tests_shadow"] > 0
    assert got["default"] == got["node_min1"]
