"""Host-only parts of rendering a frame in sample passes (hjr_params.sample_begin / sample_end): the boundary granule,
the "passes" key of the render option, the Python mirrors of the appended struct fields, and the pass split that hjr_render_file,
henjou_cli and Device.render_progressive use.  No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

from scene_util import ROOT, hjr
from test_device_bvh import _option_json


def chunk_spp(spp):  # csrc/hjr_layout.h: hjr_chunk_spp
    return 8 * (((spp + 7) // 8 + 63) // 64)


def n_chunks(spp):
    return (spp + chunk_spp(spp) - 1) // chunk_spp(spp)


def test_sample_granule_is_the_chunk_length():
    """hjr_sample_granule(spp) == hjr_chunk_spp(spp), or spp when the frame is one chunk, for spp 1 ... 5000."""
    assert hjr.sample_granule(0) == 0
    for spp in range(1, 5001):
        want = spp if n_chunks(spp) == 1 else chunk_spp(spp)
        assert hjr.sample_granule(spp) == want, spp
    assert [hjr.sample_granule(s) for s in (8, 256, 512, 1024, 4096)] == [8, 8, 8, 16, 64]


def test_render_option_parses_passes(tmp_path):
    """"Henjou_HIP": {"passes": N} sets hjr_render_option.passes (default 1); anything but an integer in [1, 64] is rejected."""
    assert hjr.load_render_option(_option_json(tmp_path, None)).passes == 1
    assert hjr.load_render_option(_option_json(tmp_path, {"seed": 3})).passes == 1
    for n in (1, 4, 64):
        assert hjr.load_render_option(_option_json(tmp_path, {"passes": n})).passes == n
    for bad in (0, 65, -1, 1.5, "2", True):
        with pytest.raises(hjr.HjrError, match="passes"):
            hjr.load_render_option(_option_json(tmp_path, {"passes": bad}))


def test_python_mirrors_match_the_c_structs(tmp_path):
    """Field offsets of the ctypes mirrors equal the C header's, and the new fields were appended (after the old last field)."""
    src = tmp_path / "off.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "henjou_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\\n", offsetof(hjr_params, flags), offsetof(hjr_params, sample_begin), offsetof(hjr_params, sample_end),
           sizeof(hjr_params), offsetof(hjr_render_option, device_bvh_opt), offsetof(hjr_render_option, passes), sizeof(hjr_render_option));
    return 0;
}
""")
    exe = str(tmp_path / "off")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    flags, sb, se, psize, dbo, passes, osize = map(int, subprocess.check_output([exe]).split())
    assert hjr.Params.flags.offset == flags and C.sizeof(hjr.Params) == flags + 4  # the layout before this change
    assert hjr.ParamsV2.sample_begin.offset == sb == flags + 4
    assert hjr.ParamsV2.sample_end.offset == se == sb + 4
    assert C.sizeof(hjr.ParamsV2) == psize
    assert hjr.RenderOption.device_bvh_opt.offset == dbo
    assert hjr.RenderOption.passes.offset == passes == dbo + 4
    assert C.sizeof(hjr.RenderOption) == osize
    p = hjr.make_params(8, 8, 16, {"pos": [0, 0, 0], "dir": [0, 0, 1], "up": [0, 1, 0], "right": [1, 0, 0], "f": 1.0})
    assert isinstance(p, hjr.ParamsV2) and p.struct_size == psize and p.sample_begin == 0 and p.sample_end == 0


def check_split(spp, passes, g, bounds):
    assert bounds[0][0] == 0 and bounds[-1][1] == spp
    for (b0, e0), (b1, e1) in zip(bounds, bounds[1:]):
        assert e0 == b1
    for b, e in bounds:
        assert b < e and b % g == 0 and (e % g == 0 or e == spp)
    assert len(bounds) <= min(passes, (spp + g - 1) // g)


def test_pass_bounds_split():
    """Device.render_progressive's split (hjr.pass_bounds, the rule hjr_render_file / henjou_cli apply to "passes"): pass k ends at
    k * spp / N rounded down to the granule, the last at spp, and passes that come out empty are dropped."""
    assert hjr.pass_bounds(16, 4, granule=8) == [(0, 8), (8, 16)]  # render_option_c1.json (16 spp = 2 chunks) with "passes": 4
    assert hjr.pass_bounds(16, 1, granule=8) == [(0, 16)]
    assert hjr.pass_bounds(64, 8, granule=8) == [(0, 8), (8, 16), (16, 24), (24, 32), (32, 40), (40, 48), (48, 56), (56, 64)]
    assert hjr.pass_bounds(100, 3, granule=8) == [(0, 32), (32, 64), (64, 100)]
    assert hjr.pass_bounds(8, 4, granule=8) == [(0, 8)]  # one chunk: the whole frame
    assert hjr.pass_bounds(4, 64, granule=4) == [(0, 4)]
    assert hjr.pass_bounds(1024, 64, granule=16) == [(16 * k, 16 * k + 16) for k in range(64)]
    assert hjr.pass_bounds(256, 32, granule=8) == [(8 * k, 8 * k + 8) for k in range(32)]
    for spp in (1, 7, 8, 9, 16, 48, 100, 256, 513, 1000, 1024, 4096, 5000):
        g = chunk_spp(spp) if n_chunks(spp) > 1 else spp
        for passes in (1, 2, 3, 4, 5, 8, 32, 64):
            check_split(spp, passes, g, hjr.pass_bounds(spp, passes, granule=g))
    for bad in (0, 65):
        with pytest.raises(ValueError):
            hjr.pass_bounds(16, bad, granule=8)
