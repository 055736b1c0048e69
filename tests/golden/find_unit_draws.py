"""Finds the sample streams of tests/shading_cases.py::UNIT_DRAWS: seeds with which some sample of a 32 x 32 frame at 32 spp, frame 1,
draws exactly 1.0 from cmj_1d at a given depth of its stream (about one draw in 4e7 does).  Restates hjo_xxhash32_u4 / hjo_cmj of
oracle/hjr_oracle.c on numpy uint32 arrays (checked against the library on the first seed) and walks the seeds in order.

    python tests/golden/find_unit_draws.py                 # the search UNIT_DRAWS came from: depth 2 over seeds 1 .. 9000, depths 4
                                                           # and 5 over seeds 1 .. 3000 (4.9e8 draws, some minutes)
    python tests/golden/find_unit_draws.py 2 940 950       # one depth, seeds [940, 950)

After a change of the sampler: run it, put the seeds it prints into UNIT_DRAWS and record the branch counts again."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle_binding as ob  # noqa: E402

W, H, SPP, FRAME = 32, 32, 32, 1
U32 = np.uint32


def rotl17(h):
    return (h << U32(17)) | (h >> U32(15))


def xxhash32_u4(px, py, pz, pw):
    P2, P3, P4, P5 = U32(2246822519), U32(3266489917), U32(668265263), U32(374761393)
    h = pw + P5 + px * P3
    h = P4 * rotl17(h)
    h = h + py * P3
    h = P4 * rotl17(h)
    h = h + pz * P3
    h = P4 * rotl17(h)
    h = P2 * (h ^ (h >> U32(15)))
    h = P3 * (h ^ (h >> U32(13)))
    return h ^ (h >> U32(16))


def permute(i, l, p):
    """hjo_cmj_permute for l a power of two (its rejection loop never repeats then)"""
    w = U32(l - 1)
    i = i ^ p; i = i * U32(0xe170893d)
    i = i ^ (p >> U32(16))
    i = i ^ ((i & w) >> U32(4))
    i = i ^ (p >> U32(8)); i = i * U32(0x0929eb3f)
    i = i ^ (p >> U32(23))
    i = i ^ ((i & w) >> U32(1)); i = i * (U32(1) | (p >> U32(27)))
    i = i * U32(0x6935fa69)
    i = i ^ ((i & w) >> U32(11)); i = i * U32(0x74dcb303)
    i = i ^ ((i & w) >> U32(2)); i = i * U32(0x9e501cc3)
    i = i ^ ((i & w) >> U32(2)); i = i * U32(0xc860a3df)
    i = i & w
    i = i ^ (i >> U32(5))
    return (i + p) % U32(l)


def randfloat(i, p):
    i = i ^ p
    i = i ^ (i >> U32(17)); i = i ^ (i >> U32(10)); i = i * U32(0xb36534e5)
    i = i ^ (i >> U32(12)); i = i ^ (i >> U32(21)); i = i * U32(0x93fc4795)
    i = i ^ U32(0xdf6e307f)
    i = i ^ (i >> U32(17)); i = i * (U32(1) | (p >> U32(18)))
    return i.astype(np.float32) * np.float32(1.0 / 4294967808.0)


def cmj_x(index, scramble):
    """the x coordinate of hjo_cmj (CMJ_M = CMJ_N = 4), float32 arithmetic in the oracle's order"""
    index = permute(index, 16, scramble * U32(0x51633e2d))
    sy = permute(index // U32(4), 4, scramble * U32(0x63d83595))
    jx = randfloat(index, scramble * U32(0xa399d265))
    f4 = np.float32(4)
    return ((index % U32(4)).astype(np.float32) + (sy.astype(np.float32) + jx) / f4) / f4


def draws(seed, depth):
    """cmj_1d of every (pixel, sample) of the frame at `depth`: float32 [W * H, SPP]"""
    pix = np.arange(W * H, dtype=U32)[:, None]
    n = (U32(FRAME * SPP) + np.arange(SPP, dtype=U32))[None, :]
    scramble = xxhash32_u4(n // U32(16), pix, U32(depth), U32(seed))
    return cmj_x(np.broadcast_to(n % U32(16), scramble.shape), scramble)


def check_against_library(seed, depth):
    u = draws(seed, depth)
    L = ob.lib()
    out = (ob.C.c_float * 2)()
    for pix, s in ((0, 0), (5, 17), (W * H - 1, SPP - 1), (333, 8)):
        n = FRAME * SPP + s
        L.hjo_cmj(n % 16, L.hjo_xxhash32_u4(n // 16, pix, depth, seed), out)
        assert np.float32(out[0]) == u[pix, s], (pix, s, out[0], u[pix, s])


def search(depth, seed0, seed1):
    found = []
    with np.errstate(over="ignore"):  # uint32 arithmetic wraps on purpose
        check_against_library(seed0, depth)
        for seed in range(seed0, seed1):
            u = draws(seed, depth)
            for pix, s in np.argwhere(u == np.float32(1.0)):
                print("seed %d depth %d: pixel (%d, %d) sample %d" % (seed, depth, pix % W, pix // W, s), flush=True)
                found.append((seed, depth))
    print("depth %d, seeds [%d, %d): %.3g draws, %d of them 1.0" % (depth, seed0, seed1, (seed1 - seed0) * W * H * SPP, len(found)))
    return found


if __name__ == "__main__":
    if len(sys.argv) == 4:
        search(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]))
    else:
        search(2, 1, 9001); search(4, 1, 3001); search(5, 1, 3001)
