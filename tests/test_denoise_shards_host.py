"""Gathered shards -> frames on the host (hjr_assemble_shards, DESIGN.md §7 "Denoise modes"): the step that turns the N blocks of up to four
AOVs rank 0 holds after the gather of a multi-GPU frame into the frames the Denoise filter reads.  Bit for bit against N applications of
hjr_unpack_tiles per float4 AOV and, for the one-float variance, against the Python tile mask; every null / non-null combination of the AOVs;
the argument rule; a stand-alone AddressSanitizer / UBSan program in which everything that must not be read is poisoned; the struct against
the header text.  No GPU needed."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from scene_util import ROOT, hjr

SHAPES = [(75, 41, 1), (75, 41, 3), (9, 17, 3), (8, 8, 4), (75, 41, 61), (64, 64, 8), (1920, 1080, 8)]  # (8, 8, 4), (75, 41, 61): ranks without a tile
AOVS = ("color", "albedo", "normal", "variance")
SENTINEL = np.float32(-7.0)


def gathered(w, h, n, extra_stride=0, seed=0):
    """One gathered buffer (float32, NaN everywhere a pixel is not: edge-tile lanes outside the image, padding behind a rank's last tile,
    slack of a larger rank_stride), its layout, and per AOV the list of every rank's block as the packers produce it."""
    off, stride = hjr.shards_layout(w, h, n)
    stride += extra_stride
    rng = np.random.default_rng(seed + 1000 * n + w)
    frames = {k: rng.random((h, w, 4), dtype=np.float32) for k in AOVS}  # (the variance travels in channel 0 of its frame)
    ones = np.ones((h, w, 4), dtype=np.float32)
    buf = np.full(stride * n // 4, np.nan, dtype=np.float32)
    blocks = {k: [] for k in AOVS}
    for r in range(n):
        inside = hjr.pack_tiles(ones, r, n)[..., 0] == 1.0  # [owned tile][64]: the slot has a pixel
        for k in AOVS:
            p = hjr.pack_tiles(frames[k], r, n)
            p[~inside] = np.nan
            blk = p[..., 0].copy() if k == "variance" else p
            blocks[k].append(blk)
            o = (r * stride + off[k]) // 4
            buf[o:o + blk.size] = blk.ravel()
    return buf, off, stride, frames, blocks


def expected(w, h, n, frames, blocks, k):
    if k == "variance":  # the Python mask restated for one float: rank r's pixels, tile by tile in id order, are its block's in-image slots
        want = np.full((h, w), SENTINEL, dtype=np.float32)
        tiles_x = (w + 7) // 8
        for r in range(n):
            m = hjr.owned_tile_mask(w, h, r, n)
            assert np.array_equal(np.isnan(blocks[k][r]), ~np.isfinite(blocks[k][r]))
            ty, tx = np.nonzero(m[::8, ::8])
            order = np.argsort(ty * tiles_x + (tx + ty) % tiles_x)
            for i, j in enumerate(order):
                y0, x0 = 8 * ty[j], 8 * tx[j]
                t = blocks[k][r][i].reshape(8, 8)[:min(8, h - y0), :min(8, w - x0)]
                want[y0:y0 + t.shape[0], x0:x0 + t.shape[1]] = t
        assert np.array_equal(want, frames[k][..., 0])
        return want
    want = np.full((h, w, 4), SENTINEL, dtype=np.float32)
    for r in range(n):
        if blocks[k][r].shape[0]:
            hjr.unpack_tiles(blocks[k][r], want, r, n)
    return want


def assemble_raw(s, w, h, outs):
    return hjr.lib().hjr_assemble_shards(C.byref(s), w, h, *[None if o is None else o.ctypes.data for o in outs])


def new_outputs(w, h, present):
    return [None if k not in present else np.full((h, w, 4) if k != "variance" else (h, w), SENTINEL, dtype=np.float32) for k in AOVS]


@pytest.fixture(scope="module")
def cases():
    return {}


def case(cases, w, h, n, extra=0):
    key = (w, h, n, extra)
    if key not in cases:
        g = gathered(w, h, n, extra)
        cases[key] = g + ({k: expected(w, h, n, g[3], g[4], k) for k in AOVS},)
    return cases[key]


@pytest.mark.parametrize("w,h,n", SHAPES)
def test_host_assemble_equals_unpack_tiles_per_rank(cases, w, h, n):
    buf, off, stride, frames, blocks, want = case(cases, w, h, n)
    s = hjr.make_shards(buf.ctypes.data, n, stride, off)
    outs = new_outputs(w, h, AOVS)
    assert assemble_raw(s, w, h, outs) == 0, hjr.lib().hjr_last_error()
    for k, o in zip(AOVS, outs):
        assert not np.isnan(o).any() and not (o == SENTINEL).any(), k  # every pixel written, no padding read
        assert np.array_equal(o, want[k]), k
    got = hjr.assemble_shards(s, w, h)  # the glue's form
    assert all(np.array_equal(a, b) for a, b in zip(got, outs))


def test_rank_stride_larger_than_needed(cases):
    w, h, n = 75, 41, 3
    buf, off, stride, frames, blocks, want = case(cases, w, h, n, 4096 + 16)
    assert stride == hjr.shards_layout(w, h, n)[1] + 4096 + 16
    got = hjr.assemble_shards(hjr.make_shards(buf.ctypes.data, n, stride, off), w, h)
    for k, o in zip(AOVS, got):
        assert np.array_equal(o, want[k]), k


@pytest.mark.parametrize("w,h,n", [(75, 41, 3), (9, 17, 3), (8, 8, 4), (75, 41, 61)])
def test_every_combination_of_present_aovs(cases, w, h, n):
    buf, off, stride, frames, blocks, want = case(cases, w, h, n)
    for m in range(1, 5):
        for present in itertools.combinations(AOVS, m):
            s = hjr.make_shards(buf.ctypes.data, n, stride, {k: off[k] for k in present})
            outs = new_outputs(w, h, present)
            assert assemble_raw(s, w, h, outs) == 0, (present, hjr.lib().hjr_last_error())
            for k, o in zip(AOVS, outs):
                assert (o is None) == (k not in present)
                if o is not None:
                    assert np.array_equal(o, want[k]), (present, k)


def test_argument_errors(cases):
    w, h, n = 75, 41, 3
    buf, off, stride, frames, blocks, want = case(cases, w, h, n)
    full = lambda: hjr.make_shards(buf.ctypes.data, n, stride, off)  # noqa: E731
    ERR_ARG = -1
    for k in AOVS:  # an output without its source, a source without its output
        s = hjr.make_shards(buf.ctypes.data, n, stride, {a: off[a] for a in AOVS if a != k})
        outs = new_outputs(w, h, AOVS)
        assert assemble_raw(s, w, h, outs) == ERR_ARG, k
        assert all((o == SENTINEL).all() for o in outs), "an output was written by a refused call"
        assert assemble_raw(full(), w, h, new_outputs(w, h, [a for a in AOVS if a != k])) == ERR_ARG, k
    assert assemble_raw(hjr.make_shards(buf.ctypes.data, n, stride, {}), w, h, new_outputs(w, h, ())) == ERR_ARG  # no AOV at all
    outs = new_outputs(w, h, AOVS)
    for bad in ({"world_size": 0}, {"rank_stride": stride + 8}, {"rank_stride": hjr.owned_tiles(w, h, 0, n) * 1024 - 16}, {"rank_stride": 0}, {"struct_size": 0}):
        s = full()
        for a, v in bad.items():
            setattr(s, a, v)
        assert assemble_raw(s, w, h, outs) == ERR_ARG, bad
    assert b"struct_size" in hjr.lib().hjr_last_error()
    assert assemble_raw(full(), 0, h, outs) == ERR_ARG and assemble_raw(full(), w, 0, outs) == ERR_ARG
    assert hjr.lib().hjr_assemble_shards(None, w, h, *[o.ctypes.data for o in outs]) == ERR_ARG
    s = full()
    s.color += 4  # a float4 block that is not 16-byte aligned
    assert assemble_raw(s, w, h, outs) == ERR_ARG
    s = full()
    s.variance += 2  # a float block that is not 4-byte aligned
    assert assemble_raw(s, w, h, outs) == ERR_ARG
    assert all((o == SENTINEL).all() for o in outs)
    # world_size 1 has no second block: any multiple of 16 is a valid stride, 0 included
    buf1, off1, stride1, _, _, want1 = case(cases, 75, 41, 1)
    s = hjr.make_shards(buf1.ctypes.data, 1, 0, off1)
    assert all(np.array_equal(o, want1[k]) for k, o in zip(AOVS, hjr.assemble_shards(s, 75, 41)))
    # a caller with a shorter (older) struct: no variance field -> colour, albedo, normal only
    short = hjr.Shards.variance.offset
    s = full()
    s.struct_size = short
    s.variance = 0xdead0  # behind struct_size: must not be looked at
    outs = new_outputs(w, h, AOVS[:3])
    assert assemble_raw(s, w, h, outs) == 0
    assert np.array_equal(outs[0], want["color"])


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shards") / "assemble_shards_test")
    host = os.path.join(ROOT, "henjou-renderer_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "native", "assemble_shards_test.cpp"), os.path.join(host, "capi.cpp"), os.path.join(host, "loaders.cpp"),
                           os.path.join(host, "image_io.cpp"), os.path.join(host, "jpeg.cpp"), "-o", exe, "-lz", "-lpthread"])
    return exe


@pytest.mark.parametrize("w,h,n", SHAPES + [(1920, 1080, 7)])
def test_host_assemble_under_asan_ubsan_with_padding_poisoned(asan_exe, w, h, n):
    """tests/native/assemble_shards_test.cpp with host/capi.cpp compiled in: the gathered buffer is allocated to the byte and every slot
    without a pixel is poisoned, so a read of padding ends the program.  (1920 x 1080 splits evenly over 8 ranks; over 7 it does not.)"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([asan_exe, str(w), str(h), str(n)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    assert "assemble_shards_test ok" in p.stdout
    if w % 8 or h % 8 or ((w // 8) * (h // 8)) % n:  # a ragged shape: there is something to trap
        assert " 0 poisoned" not in p.stdout


def test_struct_layout_matches_the_header_and_symbols_are_exported():
    text = open(os.path.join(ROOT, "include", "henjou_hip.h")).read()
    body = re.search(r"typedef struct hjr_shards \{(.*?)\} hjr_shards;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"uint32_t": 4, "uint64_t": 8, "const void*": 8}
    at, fields = 0, []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        ctype, name = re.match(r"(uint32_t|uint64_t|const void\*)\s*(\w+)$", decl).groups()
        at = (at + sizes[ctype] - 1) // sizes[ctype] * sizes[ctype]
        fields.append((name, at, sizes[ctype]))
        at += sizes[ctype]
    assert [f[0] for f in fields] == ["struct_size", "world_size", "rank_stride", "color", "albedo", "normal", "variance"]
    assert [n for n, _ in hjr.Shards._fields_] == [f[0] for f in fields]
    for name, offset, size in fields:
        fld = getattr(hjr.Shards, name)
        assert (fld.offset, fld.size) == (offset, size), name
    assert C.sizeof(hjr.Shards) == (at + 7) // 8 * 8 == 48
    assert hjr.Shards().struct_size == 48
    exported = os.popen("nm -D --defined-only %s" % hjr.LIB_PATH).read()
    for sym in ("hjr_assemble_shards", "hjr_assemble_shards_device", "hjr_denoise_shards_device"):
        assert re.search(r" T %s$" % sym, exported, re.M), sym
        assert hasattr(hjr.lib(), sym)
    for sym in ("hjr_assemble_shards", "hjr_assemble_shards_device", "hjr_denoise_shards_device"):  # declared where callers look for them
        assert re.search(r"^int %s\(" % sym, text, re.M), sym
