"""C-ABI hygiene (no GPU): libhenjou_hip.so loads, exports every symbol include/henjou_hip.h declares, struct sizes match
the Python mirrors, device entry points fail loudly without an MI355X, and the host output stage (PNG, sRGB) works."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_binding as ob
from scene_util import Cornell, entry, hjr

HEADER = os.path.join(entry.ROOT, "include", "henjou_hip.h")


def declared_symbols():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(hjr_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    L = hjr.lib()
    syms = declared_symbols()
    assert len(syms) >= 20 and "hjr_render_device" in syms and "hjr_scene_load_gltf" in syms and "hjr_trace_rays" in syms
    for s in syms:
        assert hasattr(L, s), "libhenjou_hip.so does not export " + s


def test_struct_layouts_match_header():
    assert C.sizeof(hjr.Material) == 80 and hjr.MATERIAL_DTYPE.itemsize == 80 and C.sizeof(hjr.Texture) == 24
    assert C.sizeof(hjr.Camera) == 52
    assert C.sizeof(hjr.Params) == 4 + 6 * 4 + 52 + 12 + 4 + 12
    assert C.sizeof(hjr.Stats) == 8 + 10 * 8 + 16 + 16 + 8 + 8 + 96
    assert C.sizeof(hjr.SceneView) == 8 * 4 + 13 * 8
    # hjr_ray / hjr_ray_result of the ray-batch test hook: 32 bytes each, fields where the header puts them
    assert hjr.RAY_DTYPE.itemsize == 32 and [hjr.RAY_DTYPE.fields[k][1] for k in ("o", "tmax", "d", "valid")] == [0, 12, 16, 28]
    assert hjr.RAY_RESULT_DTYPE.itemsize == 32 and [hjr.RAY_RESULT_DTYPE.fields[k][1] for k in ("occluded", "prim", "k", "t", "b1", "b2", "status", "pad")] == list(range(0, 32, 4))
    hdr = open(HEADER).read()
    assert "typedef struct hjr_ray { float o[3]; float tmax; float d[3]; uint32_t valid; } hjr_ray;" in hdr
    assert "typedef struct hjr_ray_result { uint32_t occluded, prim, k; float t, b1, b2; uint32_t status, pad; } hjr_ray_result;" in hdr
    for t in (hjr.Params, hjr.Stats, hjr.SceneView, hjr.RenderOption): # sized structs: struct_size leads and is set on construction
        assert t.struct_size.offset == 0 and t().struct_size == C.sizeof(t)


def test_stack16_encoding_roundtrips_every_ref_the_builder_can_emit():
    """the 16-bit traversal-stack entry keeps a 2-bit triangle count; host/frame.cpp only admits trees with
    leaves of <= 3 triangles, < 8192 triangles and < 32768 inner nodes to that layout, and every such ref must survive."""
    assert hjr.lib().hjr_selftest_stack16() == 0


def test_no_silent_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is not reachable")
    with pytest.raises(hjr.HjrError) as e:
        hjr.Device(0)
    assert "no CPU fallback" in str(e.value)
    L = hjr.lib()
    assert L.hjr_render(None, None, None, None, None) != 0
    assert L.hjr_upload_scene(None, None) != 0
    assert L.hjr_render_file(b"/nonexistent/render_option.json", 0) != 0
    assert b"not found" in L.hjr_last_error()


def test_product_does_not_link_the_oracle():
    out = os.popen("nm -D --undefined-only %s" % hjr.LIB_PATH).read()
    assert "hjo_" not in out
    srcs = []
    for root, _, files in os.walk(hjr.PKG_DIR):
        for f in files:
            if f.endswith((".cpp", ".hpp", ".h", ".hip", ".py")) and "build" not in root:
                srcs.append(os.path.join(root, f))
    for f in srcs:
        t = open(f).read()
        assert "hjr_oracle" not in t and "oracle_binding" not in t, f


def test_png_roundtrip_and_flip(tmp_path):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (37, 53, 4), dtype=np.uint8)
    p = str(tmp_path / "a.png")
    hjr.write_png(p, img, flip_y=False)
    back = hjr.load_png(p)
    assert np.array_equal(back, img)
    hjr.write_png(p, img, flip_y=True)  # row 0 at the bottom, as the OptiX SDK's saveImage does
    assert np.array_equal(hjr.load_png(p), img[::-1])
    from PIL import Image
    assert np.array_equal(np.array(Image.open(p).convert("RGBA")), img[::-1])
    # decoder: filters chosen by another encoder, RGB and grey inputs
    Image.fromarray(img[..., :3]).save(str(tmp_path / "rgb.png"), optimize=True)
    assert np.array_equal(hjr.load_png(str(tmp_path / "rgb.png"))[..., :3], img[..., :3])
    Image.fromarray(img[..., 0]).save(str(tmp_path / "g.png"))
    g = hjr.load_png(str(tmp_path / "g.png"))
    assert np.array_equal(g[..., 0], img[..., 0]) and np.array_equal(g[..., 1], img[..., 0]) and (g[..., 3] == 255).all()
    with pytest.raises(hjr.HjrError):
        hjr.load_png(str(tmp_path / "missing.png"))
    (tmp_path / "junk.png").write_bytes(b"not a png at all")
    with pytest.raises(hjr.HjrError):
        hjr.load_png(str(tmp_path / "junk.png"))


def test_srgb_stage_matches_oracle():
    rng = np.random.default_rng(2)
    px = rng.uniform(0, 1.5, (64, 4)).astype(np.float32)
    px[0, :3] = (0.0, 0.0031308, 1.0)
    px[1, :3] = (-1.0, np.nan, 1e30)
    a = hjr.float4_to_srgb8(px)
    b = np.zeros((64, 4), np.uint8)
    ob.lib().hjo_float4_to_srgb8(px.ctypes.data, b.ctypes.data, 64)
    assert np.array_equal(a, b)
    assert list(a[1, :3]) == [0, 0, 255] and a[0, 2] == 255


def test_tile_ownership_partitions_the_frame():
    for (w, h, R) in [(1920, 1080, 8), (200, 120, 3), (7, 5, 2), (64, 64, 5)]:
        acc = np.zeros((h, w), np.int32)
        for r in range(R):
            acc += hjr.owned_tile_mask(w, h, r, R)
        assert (acc == 1).all()
        counts = [int(hjr.owned_tile_mask(w, h, r, R).sum()) for r in range(R)]
        if w * h > 4096:
            assert max(counts) - min(counts) <= 64 * 2 + (w % 8 + h % 8) * max(w, h)


def test_tonemappers_match_oracle_and_formulae():
    """kernel/color.h: Uchimura (:10-53) and ACES (:55-63) on the preview buffer, then the sRGB stage."""
    L = ob.lib()
    xs = np.concatenate([np.linspace(0, 4, 400), [0.22, 0.62, 1e-6, 100.0]]).astype(np.float32)
    px = np.zeros((len(xs), 4), np.float32)
    px[:, 0] = xs
    px[:, 1] = xs * 0.5
    px[:, 2] = xs[::-1]
    px[:, 3] = 1
    for mode in (hjr.TONEMAP_NONE, hjr.TONEMAP_UCHIMURA, hjr.TONEMAP_ACES):
        a = hjr.tonemap_to_srgb8(px, mode)
        b = np.zeros_like(a)
        L.hjo_tonemap_to_srgb8(px.ctypes.data, b.ctypes.data, len(xs), mode)
        assert np.array_equal(a, b)
    assert np.array_equal(hjr.tonemap_to_srgb8(px, hjr.TONEMAP_NONE), hjr.float4_to_srgb8(px))

    def aces(x):
        return np.clip((x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14), 0, 1)
    for x in (0.0, 0.18, 1.0, 3.0):
        assert abs(L.hjo_tonemap(x, 2) - aces(x)) < 1e-6
    # Uchimura with P=1,a=1,m=0.22,l=0.4: toe below m, linear up to m+l0, shoulder towards P
    assert abs(L.hjo_tonemap(0.0, 1)) < 1e-7
    assert abs(L.hjo_tonemap(0.5, 1) - 0.5) < 1e-6          # linear section [0.22, 0.532]... and blend weights sum to 1
    assert 0.9 < L.hjo_tonemap(2.0, 1) < 1.0 and L.hjo_tonemap(50.0, 1) <= 1.0
    ys = np.array([L.hjo_tonemap(float(x), 1) for x in np.linspace(0, 5, 200)])
    assert np.all(np.diff(ys) >= -1e-6)
    with pytest.raises(hjr.HjrError):
        hjr.tonemap_to_srgb8(px, 7)


def test_library_reads_no_environment_variable():
    """The shipped library's behaviour depends on its arguments and hjr_set_option only: no getenv in its dynamic symbol table
    (round 2 read ~15 tuning knobs from the caller's environment inside the launch path)."""
    out = os.popen("nm -D --undefined-only %s" % hjr.LIB_PATH).read()
    assert "getenv" not in out, [l for l in out.splitlines() if "getenv" in l]
