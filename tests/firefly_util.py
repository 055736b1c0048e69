"""The firefly clamp (option "firefly_clamp"; include/henjou_hip.h "Firefly clamp", DESIGN.md §4 rule 9) restated in numpy float32, and the
oracle's colour chunk sums it is applied to.  No GPU needed; tools may import it.

Every operation below is one IEEE fp32 operation in the order the header writes it, so the result equals the device's bit for bit."""
import numpy as np

f32 = np.float32
EPS = f32(1e-3)  # HJR_FIREFLY_EPS


def granule_of(spp):
    """hjr_sample_granule(spp) (csrc/hjr_layout.h): the chunk length, or spp itself for a frame of a single chunk."""
    n8 = (spp + 7) // 8
    g = 8 * ((n8 + 63) // 64)
    return g if (spp + g - 1) // g > 1 else spp


def lower_median(y):
    """The value of rank (m - 1) // 2 in ascending order along axis 0 of y [m, ...]."""
    return np.sort(np.asarray(y, f32), axis=0)[(y.shape[0] - 1) // 2]


def plain_sum(chunk):
    """Chunk sums [n, ..., 3] added in chunk order from +0.0f: the plain frame's running sum."""
    a = np.zeros(chunk.shape[1:], f32)
    for k in range(chunk.shape[0]):
        a = a + chunk[k]
    return a


def firefly_rule(chunk, g, spp, kappa):
    """chunk: float32 [n_chunks, ..., 3], the colour chunk sums of every pixel as stored (the partial last chunk, if spp is no multiple of
    g, is the last one).  Returns (rgb mean float32 [..., 3], number of scaled (pixel, chunk) pairs, bool [...] pixels with a scaled chunk)."""
    chunk = np.ascontiguousarray(chunk, f32)
    n, m = chunk.shape[0], spp // g
    r = spp - m * g
    assert n == m + (1 if r else 0), "chunk sums do not match spp / g"
    touched = np.zeros(chunk.shape[1:-1], bool)
    inv = f32(1) / f32(spp)
    if not (kappa > 0 and m >= 4):  # step 1: the plain frame
        return plain_sum(chunk) * inv, 0, touched
    y = (chunk[..., 0] + chunk[..., 1]) + chunk[..., 2]
    med = lower_median(y[:m])                    # step 2
    lim = f32(kappa) * med + EPS * f32(g)        # step 3
    lim_r = lim * (f32(r) / f32(g))              # step 4
    a = np.zeros(chunk.shape[1:], f32)
    count = 0
    for k in range(n):                           # step 5
        L = lim if k < m else lim_r
        over = y[k] > L
        s = np.ones_like(L)
        np.divide(L, y[k], out=s, where=over)
        a = a + chunk[k] * s[..., None]
        count += int(over.sum())
        touched |= over
    return a * inv, count, touched               # step 6


def moved_camera(camera, x):
    """A copy of an hjr Camera with pos.x replaced."""
    c = type(camera).from_buffer_copy(camera)
    c.pos[0] = x
    return c


_chunks = {}


def oracle_color_chunks(cornell, w, h, spp, integrator=0, camera=None, seed=1):
    """Colour chunk sums of the oracle's per-sample values, [n_chunks][h][w][3] float32: the samples of a chunk added in sample order from
    +0.0f, as the render kernels add them (tests/test_gpu_variance.py::chunk_sums, colour only, the adds vectorised over the pixels).
    Returns (chunk, g).  Cached per argument set; callers must not modify the array."""
    import oracle_binding as ob
    cam = camera if camera is not None else cornell.camera
    key = (id(cornell), w, h, spp, integrator, tuple(cam.pos), seed)
    if key not in _chunks:
        g = granule_of(spp)
        osc = ob.OracleScene(cornell.arrays, ob.MATH_PORTABLE)
        op = ob.make_params(w, h, spp, cam.as_dict(), seed=seed, integrator=integrator, sky=tuple(cornell.opt.scene_sky_default),
                            ibl_intensity=cornell.opt.IBL_intensity)
        n = (spp + g - 1) // g
        chunk = np.zeros((n, h, w, 3), f32)
        plane = np.zeros((h, w, 3), f32)
        r = ob.F3()
        a = ob.F3()
        nn = ob.F3()
        import ctypes as C
        sample = ob.lib().hjo_sample
        ctx, pp = osc.ctx, C.byref(op)
        for s in range(spp):
            for y in range(h):
                for x in range(w):
                    sample(ctx, pp, x, y, s, r, a, nn)
                    plane[y, x] = r
            chunk[s // g] = chunk[s // g] + plane
        chunk.setflags(write=False)
        _chunks[key] = (chunk, g)
    return _chunks[key]


def frame_of(rgb):
    """float4 frame [h, w, 4] with alpha 1 from an rgb mean [h, w, 3]."""
    out = np.ones(rgb.shape[:-1] + (4,), f32)
    out[..., :3] = rgb
    return out
