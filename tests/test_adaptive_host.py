"""Host-only parts of adaptive sampling (hjr_set_adaptive): the Python mirrors of hjr_adaptive / hjr_adaptive_state and of
the two fields appended to hjr_render_option, and the "noise_threshold" / "min_samples" keys of the render option.  No GPU needed."""
import ctypes as C
import json
import os
import subprocess

import pytest

from scene_util import ROOT, hjr
from test_device_bvh import _option_json


def test_python_mirrors_match_the_c_structs(tmp_path):
    """Offsets and sizes of hjr_adaptive, hjr_adaptive_state and the appended hjr_render_option fields equal the C header's, and
    hjr_params did not grow: the settings live in the context, sizeof(hjr_params) == sizeof(ParamsV2)."""
    src = tmp_path / "off.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "henjou_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu ", offsetof(hjr_adaptive, struct_size), offsetof(hjr_adaptive, noise_threshold), offsetof(hjr_adaptive, min_samples), sizeof(hjr_adaptive));
    printf("%zu %zu %zu %zu %zu ", offsetof(hjr_adaptive_state, owned_tiles), offsetof(hjr_adaptive_state, active_tiles), offsetof(hjr_adaptive_state, sample_end),
           offsetof(hjr_adaptive_state, samples_rendered), sizeof(hjr_adaptive_state));
    printf("%zu %zu %zu %zu %zu\\n", offsetof(hjr_render_option, passes), offsetof(hjr_render_option, noise_threshold), offsetof(hjr_render_option, min_samples),
           sizeof(hjr_render_option), sizeof(hjr_params));
    printf("%.9g\\n", (double)HJR_ADAPTIVE_EPS);
    return 0;
}
""")
    exe = str(tmp_path / "off")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe]).decode().splitlines()
    v = list(map(int, lines[0].split()))
    A, S, O = hjr.Adaptive, hjr.AdaptiveState, hjr.RenderOption
    assert [A.struct_size.offset, A.noise_threshold.offset, A.min_samples.offset, C.sizeof(A)] == v[0:4] == [0, 4, 8, 12]
    assert [S.owned_tiles.offset, S.active_tiles.offset, S.sample_end.offset, S.samples_rendered.offset, C.sizeof(S)] == v[4:9] == [4, 8, 12, 16, 24]
    assert [O.passes.offset, O.noise_threshold.offset, O.min_samples.offset, C.sizeof(O)] == v[9:13]
    assert v[10] == v[9] + 4 and v[11] == v[10] + 4  # appended after the old last field
    assert C.sizeof(hjr.ParamsV2) == v[13]
    assert float(lines[1]) == 1e-3 or abs(float(lines[1]) - 1e-3) < 1e-9
    assert A().struct_size == 12 and S().struct_size == 24


def test_render_option_parses_noise_threshold_and_min_samples(tmp_path):
    """"Henjou_HIP": {"noise_threshold": t, "min_samples": n}: off by default; negative, non-finite and non-numeric thresholds and a
    non-integer min_samples are rejected; a threshold without "passes" splits the frame into 8 passes, and only then."""
    for extra in (None, {"seed": 3}, {"passes": 4}):
        o = hjr.load_render_option(_option_json(tmp_path, extra))
        assert o.noise_threshold == 0.0 and o.min_samples == 0
        assert o.passes == (4 if extra and "passes" in extra else 1)
    o = hjr.load_render_option(_option_json(tmp_path, {"noise_threshold": 0.08}))
    assert o.noise_threshold == C.c_float(0.08).value and o.min_samples == 0 and o.passes == 8
    o = hjr.load_render_option(_option_json(tmp_path, {"noise_threshold": 0.1, "min_samples": 96, "passes": 16}))
    assert o.noise_threshold == C.c_float(0.1).value and o.min_samples == 96 and o.passes == 16
    o = hjr.load_render_option(_option_json(tmp_path, {"noise_threshold": 0.1, "passes": 1}))
    assert o.passes == 1
    o = hjr.load_render_option(_option_json(tmp_path, {"noise_threshold": 0}))  # an explicit 0 is off: no 8-pass default
    assert o.noise_threshold == 0.0 and o.passes == 1
    o = hjr.load_render_option(_option_json(tmp_path, {"min_samples": 40}))
    assert o.noise_threshold == 0.0 and o.min_samples == 40 and o.passes == 1
    for bad in (-0.01, -1, "0.1", True, None, [0.1]):
        with pytest.raises(hjr.HjrError, match="noise_threshold"):
            hjr.load_render_option(_option_json(tmp_path, {"noise_threshold": bad}))
    # non-finite: a literal beyond double (and beyond float) range, written into the JSON text by hand
    for lit in ("1e999", "1e39"):
        ro = json.load(open(os.path.join(hjr.ASSETS, "render_option_c1.json")))
        ro["Henjou_HIP"] = {"noise_threshold": "@@"}
        path = tmp_path / "inf.json"
        path.write_text(json.dumps(ro).replace('"@@"', lit))
        with pytest.raises(hjr.HjrError):
            hjr.load_render_option(str(path))
    for bad in (1.5, -1, "32", True, 2 ** 21):
        with pytest.raises(hjr.HjrError, match="min_samples"):
            hjr.load_render_option(_option_json(tmp_path, {"noise_threshold": 0.1, "min_samples": bad}))
