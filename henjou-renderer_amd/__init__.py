"""Thin Python glue over libhenjou_hip.so (C-ABI: include/henjou_hip.h).

Python is plumbing here — tests, bench.py and the torch.distributed (RCCL) framebuffer exchange.  The product is
the C++/HIP library; this module adds no compute path and no fallback: if the library is missing or no MI355X is
present, the calls raise.

`Renderer` mirrors the reference's `class Renderer` (renderer/renderer.h:900-1318): loadRenderOption,
loadGLTFfile, build, and a per-frame render that returns the linear float4 AOVs.
"""
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("HJR_LIB") or os.path.join(PKG_DIR, "libhenjou_hip.so")  # HJR_LIB: kernel-variant experiments only
ASSETS = os.path.join(PKG_DIR, "assets")

INTEGRATOR_NEE, INTEGRATOR_PT, INTEGRATOR_MIS = 0, 1, 2
MODE_DEFAULT, MODE_DENOISE, MODE_DENOISE_UPSCALE2X, MODE_DEBUG = 0, 1, 2, 3  # render_option.h:38-43
FLAG_STATS, FLAG_ZERO_UNOWNED, FLAG_PACKED, FLAG_FAST_MATH = 1, 2, 4, 8
VARIANCE_UNKNOWN = np.float32(1e30)  # HJR_VARIANCE_UNKNOWN: fewer than two full chunks behind a pixel of the variance AOV
FRAME_NODES, FRAME_TRI_GEOM, FRAME_TRI_SHADE, FRAME_LIGHTS = 0, 1, 2, 3  # hjr_copy_frame_data


class HjrError(RuntimeError):
    pass


class Material(C.Structure):
    _fields_ = [("basecolor", C.c_float * 3), ("metallic", C.c_float), ("roughness", C.c_float),
                ("sheen", C.c_float), ("clearcoat", C.c_float), ("ior", C.c_float),
                ("transmission", C.c_float), ("emission", C.c_float * 3), ("is_light", C.c_int32),
                ("ideal_specular", C.c_int32), ("is_thinfilm", C.c_int32), ("basecolor_tex", C.c_int32),
                ("metallic_roughness_tex", C.c_int32), ("normal_tex", C.c_int32), ("emission_tex", C.c_int32),
                ("_reserved", C.c_int32)]


MATERIAL_DTYPE = np.dtype([("basecolor", "<f4", 3), ("metallic", "<f4"), ("roughness", "<f4"), ("sheen", "<f4"),
                           ("clearcoat", "<f4"), ("ior", "<f4"), ("transmission", "<f4"), ("emission", "<f4", 3),
                           ("is_light", "<i4"), ("ideal_specular", "<i4"), ("is_thinfilm", "<i4"),
                           ("basecolor_tex", "<i4"), ("metallic_roughness_tex", "<i4"), ("normal_tex", "<i4"),
                           ("emission_tex", "<i4"), ("_reserved", "<i4")])


class Texture(C.Structure):
    _fields_ = [("rgba8", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("srgb", C.c_int32),
                ("_reserved", C.c_int32)]


class _Sized(C.Structure):
    """Sized struct of the C-ABI (include/henjou_hip.h): struct_size = sizeof(this struct), set on construction (HJR_INIT)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(self)


class SceneView(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32), ("n_instances", C.c_uint32),
                ("n_materials", C.c_uint32), ("n_lights", C.c_uint32), ("n_animations", C.c_uint32),
                ("n_textures", C.c_uint32),
                ("vertices", C.c_void_p), ("normals", C.c_void_p), ("texcoords", C.c_void_p),
                ("indices", C.c_void_p), ("material_ids", C.c_void_p), ("prim_offset", C.c_void_p),
                ("geometry_index_offset", C.c_void_p), ("geometry_index_count", C.c_void_p),
                ("instance_animation_id", C.c_void_p), ("materials", C.c_void_p),
                ("light_prim_ids", C.c_void_p), ("light_prim_emission", C.c_void_p), ("textures", C.c_void_p)]


class RenderOption(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("image_width", C.c_uint32), ("image_height", C.c_uint32), ("image_name", C.c_char * 256),
                ("image_directory", C.c_char * 512), ("max_spp", C.c_uint32), ("gltf_path", C.c_char * 512),
                ("gltf_name", C.c_char * 256), ("fps", C.c_uint32), ("start_frame", C.c_uint32),
                ("end_frame", C.c_uint32), ("time_limit", C.c_float), ("allow_camera_animation", C.c_int32),
                ("camera_fov", C.c_float), ("camera_position", C.c_float * 3), ("camera_direction", C.c_float * 3),
                ("camera_animation_id", C.c_int32), ("render_mode", C.c_int32), ("ptxfile_path", C.c_char * 512),
                ("use_IBL", C.c_int32), ("IBL_path", C.c_char * 512), ("IBL_intensity", C.c_float),
                ("scene_sky_default", C.c_float * 3), ("use_date", C.c_int32), ("save_renderOption", C.c_int32),
                ("LUT_path", C.c_char * 512), ("seed", C.c_uint32), ("integrator", C.c_int32),
                ("devices", C.c_uint32), ("tile", C.c_uint32), ("serial_io", C.c_int32), ("fast_math", C.c_int32), ("force_rebuild", C.c_int32),
                ("device_bvh", C.c_int32), ("device_bvh_opt", C.c_int32), ("passes", C.c_uint32),
                ("noise_threshold", C.c_float), ("min_samples", C.c_uint32), ("denoise_variance", C.c_int32)]


class RenderOptionV2(RenderOption):
    """hjr_render_option_window: hjr_render_option (`RenderOption`, the layout up to denoise_variance) with the "Henjou_HIP" keys "window"
    [x0, y0, x1, y1] and "bucket" [bw, bh] (include/henjou_hip.h).  Both are valid callers under the sized-struct rule; load_render_option
    returns this one."""
    _fields_ = [("window", C.c_uint32 * 4), ("bucket", C.c_uint32 * 2)]


class Camera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("dir", C.c_float * 3), ("up", C.c_float * 3), ("right", C.c_float * 3),
                ("f", C.c_float)]

    def as_dict(self):
        return {"pos": list(self.pos), "dir": list(self.dir), "up": list(self.up), "right": list(self.right),
                "f": float(self.f)}


class Params(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("frame", C.c_uint32),
                ("seed", C.c_uint32), ("integrator", C.c_uint32), ("camera", Camera), ("sky", C.c_float * 3),
                ("ibl_intensity", C.c_float), ("rank", C.c_uint32), ("world_size", C.c_uint32),
                ("flags", C.c_uint32)]


class ParamsV2(Params):
    """hjr_params with the fields appended after `Params` (the layout up to flags): the sample pass of a progressive frame
    (include/henjou_hip.h; sample_end 0 = the whole frame).  Both are valid callers under the sized-struct rule; make_params returns this one."""
    _fields_ = [("sample_begin", C.c_uint32), ("sample_end", C.c_uint32)]


class ParamsV3(ParamsV2):
    """hjr_params_window: hjr_params with the render window behind it (include/henjou_hip.h: x0, y0, x1, y1 in full-frame pixels; x1 == 0 =
    the whole frame).
    A shorter caller (Params, ParamsV2) renders the whole frame; make_params returns this one when it is given a window."""
    _fields_ = [("window", C.c_uint32 * 4)]


class Stats(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("_pad0", C.c_uint32)] + [(n, C.c_uint64) for n in ("samples", "closest_rays", "shadow_rays", "box_tests_closest",
                                           "tri_tests_closest", "box_tests_shadow", "tri_tests_shadow",
                                           "shaded_hits", "light_samples", "nan_samples")] + \
               [("last_kernel_ms", C.c_float), ("bvh_nodes", C.c_uint32), ("bvh_depth", C.c_uint32),
                ("n_triangles", C.c_uint32), ("lds_mode", C.c_uint32), ("stack_need", C.c_uint32),
                ("stack_lds_entries", C.c_uint32), ("pipeline", C.c_uint32), ("stack_overflow_pushes", C.c_uint64),
                ("nan_located", C.c_uint32), ("fast_math", C.c_uint32), ("nan_where", (C.c_uint32 * 3) * 8)]

    def as_dict(self):
        names = [n for k in reversed(type(self).__mro__) for n, _ in getattr(k, "_fields_", [])]
        d = {n: (float(getattr(self, n)) if n in ("last_kernel_ms", "frame_build_ms", "bvh_sah", "bvh_topology_ms") else int(getattr(self, n)))
             for n in names if n not in ("struct_size", "_pad0", "_pad1", "_pad2", "nan_where")}
        d["nan_where"] = [tuple(int(v) for v in self.nan_where[i]) for i in range(int(self.nan_located))]  # (x, y, sample)
        return d


class StatsV2(Stats):
    """hjr_stats with the fields appended after `Stats` (the layout up to nan_where).  Both are valid callers under the sized-struct
    rule: the library writes min(struct_size, its sizeof) bytes."""
    _fields_ = [("bvh_builder", C.c_uint32), ("frame_build_ms", C.c_float)]


class StatsV3(StatsV2):
    """hjr_stats with the refit fields appended after `StatsV2` (option "device_bvh_refit")."""
    _fields_ = [("bvh_refits", C.c_uint32), ("bvh_sah", C.c_float)]


class StatsV4(StatsV3):
    """hjr_stats with the instance-tree fields appended after `StatsV3` (option "device_bvh_instances")."""
    _fields_ = [("bvh_instances", C.c_uint32), ("bvh_topology_ms", C.c_float)]


class StatsV5(StatsV4):
    """hjr_stats with the firefly-clamp counter appended after `StatsV4` (option "firefly_clamp")."""
    _fields_ = [("firefly_clamped", C.c_uint64)]


class StatsV6(StatsV5):
    """hjr_stats with the work-item length of the last launch appended after `StatsV5` (option "item_chunks")."""
    _fields_ = [("item_chunks", C.c_uint32), ("_pad1", C.c_uint32)]


class StatsV7(StatsV6):
    """hjr_stats with the deformation fields appended after `StatsV6` (hjr_set_morph, hjr_update_vertices).  Device.stats() uses this one."""
    _fields_ = [("morph_vertices", C.c_uint32), ("_pad2", C.c_uint32), ("geometry_generation", C.c_uint64)]


class MorphSet(C.Structure):
    """hjr_morph_set: one deformed vertex range of hjr_set_morph."""
    _fields_ = [("first_vertex", C.c_uint32), ("n_vertices", C.c_uint32), ("n_targets", C.c_uint32), ("first_weight", C.c_uint32),
                ("position_deltas", C.c_void_p), ("normal_deltas", C.c_void_p)]


class Morph(_Sized):
    """hjr_morph: the morph sets of a scene and their default weights (hjr_set_morph, hjr_scene_get_morph)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_sets", C.c_uint32), ("n_weights", C.c_uint32), ("_pad0", C.c_uint32), ("sets", C.c_void_p),
                ("default_weights", C.c_void_p)]


class Adaptive(_Sized):
    """hjr_adaptive: the adaptive-sampling setting of a context (hjr_set_adaptive)."""
    _fields_ = [("struct_size", C.c_uint32), ("noise_threshold", C.c_float), ("min_samples", C.c_uint32)]


class AdaptiveState(_Sized):
    """hjr_adaptive_state: the context's adaptive progressive frame after its last pass (hjr_get_adaptive_state)."""
    _fields_ = [("struct_size", C.c_uint32), ("owned_tiles", C.c_uint32), ("active_tiles", C.c_uint32), ("sample_end", C.c_uint32),
                ("samples_rendered", C.c_uint64)]


# hjr_ray / hjr_ray_result of the ray-batch test hook (hjr_trace_rays)
RAY_DTYPE = np.dtype([("o", "<f4", 3), ("tmax", "<f4"), ("d", "<f4", 3), ("valid", "<u4")])
RAY_RESULT_DTYPE = np.dtype([("occluded", "<u4"), ("prim", "<u4"), ("k", "<u4"), ("t", "<f4"), ("b1", "<f4"), ("b2", "<f4"),
                             ("status", "<u4"), ("pad", "<u4")])
TRACE_STANDALONE, TRACE_FUSED, TRACE_WAVEFRONT, TRACE_FAST_BUILD = 0, 1, 2, 0x100
TRACE_STATUS_OK, TRACE_STATUS_ROUND_CAP, TRACE_STATUS_UNTRACED = 0, 1, 2


# hjr_gbuffer_px: one record per pixel of the G-buffer pass (hjr_render_gbuffer); prim == GBUFFER_MISS and zeros elsewhere for a miss
GBUFFER_DTYPE = np.dtype([("prim", "<u4"), ("inst", "<u4"), ("t", "<f4"), ("b1", "<f4"), ("b2", "<f4"), ("pos", "<f4", 3), ("ng", "<f4", 3),
                          ("pad", "<u4")])
GBUFFER_MISS = 0xffffffff
TEMPORAL_ALPHA = np.float32(0.2)  # HJR_TEMPORAL_ALPHA
TEMPORAL_SNAP = np.float32(0.125)  # HJR_TEMPORAL_SNAP
TEMPORAL_MOMENTS_MIN = np.float32(4.0)  # HJR_TEMPORAL_MOMENTS_MIN
TEMPORAL_RESP = {"R": 2, "T0": np.float32(3.0), "T1": np.float32(6.0), "NMIN": 5, "EPS": np.float32(1e-3)}  # HJR_TEMPORAL_RESP_*


class TemporalFrame(_Sized):
    """hjr_temporal_frame: one side (previous / current frame) of hjr_temporal_accumulate."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("n_instances", C.c_uint32), ("camera", Camera),
                ("transforms12", C.c_void_p), ("inv_transforms12", C.c_void_p), ("gbuffer", C.c_void_p), ("color", C.c_void_p),
                ("variance", C.c_void_p), ("history", C.c_void_p), ("coverage", C.c_uint32)]


class Shards(_Sized):
    """hjr_shards: the gathered blocks of a multi-GPU frame as rank 0 holds them (hjr_assemble_shards / hjr_denoise_shards_device): rank r's
    block of every AOV lies r * rank_stride bytes behind rank 0's; a null pointer is an absent AOV."""
    _fields_ = [("struct_size", C.c_uint32), ("world_size", C.c_uint32), ("rank_stride", C.c_uint64), ("color", C.c_void_p),
                ("albedo", C.c_void_p), ("normal", C.c_void_p), ("variance", C.c_void_p)]


_lib = None


def lib():
    """Loads libhenjou_hip.so.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HjrError("libhenjou_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C henjou-renderer_amd`; there is no fallback path")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (soname libamdhip64.so.7) and asks for
        # it by file name, so if /opt/rocm's copy were loaded first torch would load a second runtime and then see no GPU.
        # Importing torch first makes libhenjou_hip.so's NEEDED libamdhip64.so.7 resolve to the copy torch already mapped.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.hjr_last_error.restype = C.c_char_p
        for name, args in {
            "hjr_load_render_option": [C.c_char_p, C.c_void_p],
            "hjr_load_render_option_window": [C.c_char_p, C.c_void_p],
            "hjr_scene_load_gltf": [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p],
            "hjr_scene_get_view": [C.c_void_p, C.c_void_p],
            "hjr_scene_eval_transforms": [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p],
            "hjr_scene_eval_camera": [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p],
            "hjr_scene_get_morph": [C.c_void_p, C.c_void_p],
            "hjr_scene_eval_morph_weights": [C.c_void_p, C.c_float, C.c_void_p, C.c_uint32],
            "hjr_load_png_rgba8": [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_load_hdr_rgba32f": [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_set_sky": [C.c_void_p, C.c_void_p, C.c_int, C.c_int],
            "hjr_update_vertices": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p],
            "hjr_set_morph": [C.c_void_p, C.c_void_p],
            "hjr_set_morph_weights": [C.c_void_p, C.c_void_p, C.c_uint32],
            "hjr_create": [C.c_int, C.c_void_p],
            "hjr_upload_scene": [C.c_void_p, C.c_void_p],
            "hjr_set_transforms": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32],
            "hjr_set_lut": [C.c_void_p, C.c_void_p, C.c_int, C.c_int],
            "hjr_render": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_render_device": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_render_var": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_render_device_var": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_denoise_var": [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32],
            "hjr_denoise_var_device": [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                       C.c_void_p],
            "hjr_estimate_variance": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_estimate_variance_device": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_synchronize": [C.c_void_p],
            "hjr_get_stats": [C.c_void_p, C.c_void_p],
            "hjr_preview_device": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p],
            "hjr_set_option": [C.c_void_p, C.c_char_p, C.c_int],
            "hjr_get_option": [C.c_void_p, C.c_char_p, C.c_void_p],
            "hjr_copy_frame_data": [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p],
            "hjr_float4_to_srgb8": [C.c_void_p, C.c_void_p, C.c_uint32],
            "hjr_tonemap_to_srgb8": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int],
            "hjr_write_png": [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int],
            "hjr_write_pfm": [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32],
            "hjr_render_file": [C.c_char_p, C.c_int],
            "hjr_load_image_rgba8": [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_denoise": [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32],
            "hjr_denoise_device": [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
            "hjr_render_denoised": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32],
            "hjr_pack_tiles": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p],
            "hjr_unpack_tiles": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p],
            "hjr_pack_tiles_device": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p],
            "hjr_unpack_tiles_device": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p],
            "hjr_selftest_stack16": [],
            "hjr_trace_rays": [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_set_adaptive": [C.c_void_p, C.c_void_p],
            "hjr_get_adaptive_state": [C.c_void_p, C.c_void_p],
            "hjr_copy_tile_samples": [C.c_void_p, C.c_void_p, C.c_size_t],
            "hjr_render_gbuffer": [C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_render_gbuffer_device": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_render_gbuffer_cov": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
            "hjr_render_gbuffer_cov_device": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
            "hjr_temporal_accumulate": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_temporal_accumulate_device": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_temporal_accumulate_moments": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_temporal_accumulate_moments_device": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_temporal_accumulate_response": [C.c_void_p] * 9,
            "hjr_temporal_accumulate_response_device": [C.c_void_p] * 10,
            "hjr_temporal_prior": [C.c_void_p] * 4,
            "hjr_temporal_prior_device": [C.c_void_p] * 5,
            "hjr_temporal_reset": [C.c_void_p],
            "hjr_upscale_guided": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32],
            "hjr_upscale_guided_device": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                          C.c_void_p],
            "hjr_assemble_shards": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_assemble_shards_device": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "hjr_denoise_shards_device": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
            "hjr_bucket_window": [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p],
            "hjr_blit_window": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32],
            "hjr_blit_window_device": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
        }.items():
            fn = getattr(L, name)
            fn.restype = C.c_int
            fn.argtypes = args
        L.hjr_owned_tiles.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        L.hjr_owned_tiles.restype = C.c_uint32
        L.hjr_bucket_count.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        L.hjr_bucket_count.restype = C.c_uint32
        L.hjr_sample_granule.argtypes = [C.c_uint32]
        L.hjr_sample_granule.restype = C.c_uint32
        L.hjr_scene_free.argtypes = [C.c_void_p]
        L.hjr_scene_free.restype = None
        L.hjr_destroy.argtypes = [C.c_void_p]
        L.hjr_destroy.restype = None
        L.hjr_free.argtypes = [C.c_void_p]
        L.hjr_free.restype = None
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise HjrError("%s failed (%d): %s" % (what, rc, lib().hjr_last_error().decode("utf-8", "replace")))


def _np(ptr, count, dtype):
    if not ptr or count == 0:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=count).copy()


def load_render_option(path):
    """load_json (loader/render_json_loader.h:78-228)."""
    opt = RenderOptionV2()
    _check(lib().hjr_load_render_option_window(os.fsencode(path), C.byref(opt)), "hjr_load_render_option_window")
    return opt


def load_png(path):
    p = C.c_void_p()
    w, h = C.c_int(), C.c_int()
    _check(lib().hjr_load_png_rgba8(os.fsencode(path), C.byref(p), C.byref(w), C.byref(h)), "hjr_load_png_rgba8")
    a = _np(p.value, w.value * h.value * 4, np.uint8).reshape(h.value, w.value, 4)
    lib().hjr_free(p)
    return a


def load_image(path):
    """Material texture decode: PNG or baseline JPEG by signature (hjr_load_image_rgba8) -> uint8 [h, w, 4]."""
    p = C.c_void_p()
    w, h = C.c_int(), C.c_int()
    _check(lib().hjr_load_image_rgba8(os.fsencode(path), C.byref(p), C.byref(w), C.byref(h)), "hjr_load_image_rgba8")
    a = _np(p.value, w.value * h.value * 4, np.uint8).reshape(h.value, w.value, 4)
    lib().hjr_free(p)
    return a


def load_hdr(path):
    """Radiance .hdr -> float32 [h, w, 4] (a = 0), as HDRTexture holds it (renderer/texture.h:67-88)."""
    p = C.c_void_p()
    w, h = C.c_int(), C.c_int()
    _check(lib().hjr_load_hdr_rgba32f(os.fsencode(path), C.byref(p), C.byref(w), C.byref(h)), "hjr_load_hdr_rgba32f")
    a = _np(p.value, w.value * h.value * 4, np.float32).reshape(h.value, w.value, 4)
    lib().hjr_free(p)
    return a


def write_png(path, rgba8, flip_y=True):
    a = np.ascontiguousarray(rgba8, dtype=np.uint8)
    _check(lib().hjr_write_png(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0], 1 if flip_y else 0), "hjr_write_png")


def float4_to_srgb8(rgba):
    a = np.ascontiguousarray(rgba, dtype=np.float32)
    out = np.zeros(a.shape, dtype=np.uint8)
    _check(lib().hjr_float4_to_srgb8(a.ctypes.data, out.ctypes.data, a.size // 4), "hjr_float4_to_srgb8")
    return out


TONEMAP_NONE, TONEMAP_UCHIMURA, TONEMAP_ACES = 0, 1, 2


def tonemap_to_srgb8(rgba, tonemap):
    """kernel/color.h tonemapper, then toSRGB + quantise (renderer.h:73-101)."""
    a = np.ascontiguousarray(rgba, dtype=np.float32)
    out = np.zeros(a.shape, dtype=np.uint8)
    _check(lib().hjr_tonemap_to_srgb8(a.ctypes.data, out.ctypes.data, a.size // 4, tonemap), "hjr_tonemap_to_srgb8")
    return out


class Scene:
    """Owning handle of a loaded glTF scene (SceneData, renderer/scene.h:19-36)."""

    def __init__(self, directory, filename, opt):
        self._h = C.c_void_p()
        _check(lib().hjr_scene_load_gltf(os.fsencode(directory), os.fsencode(filename), C.byref(opt), C.byref(self._h)),
               "hjr_scene_load_gltf")
        self.view = SceneView()
        _check(lib().hjr_scene_get_view(self._h, C.byref(self.view)), "hjr_scene_get_view")

    def close(self):
        if self._h:
            lib().hjr_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transforms(self, time):
        n = self.view.n_instances
        m = np.zeros((n, 12), dtype=np.float32)
        inv = np.zeros((n, 12), dtype=np.float32)
        _check(lib().hjr_scene_eval_transforms(self._h, C.c_float(time), m.ctypes.data, inv.ctypes.data),
               "hjr_scene_eval_transforms")
        return m, inv

    def camera(self, opt, time):
        cam = Camera()
        _check(lib().hjr_scene_eval_camera(self._h, C.byref(opt), C.c_float(time), C.byref(cam)), "hjr_scene_eval_camera")
        return cam

    def morph(self):
        """hjr_scene_get_morph: (sets, default_weights) in the form Device.set_morph takes (numpy copies), or ([], empty) for a file without
        morph targets.  The scene view and arrays() stay the rest pose."""
        m = Morph()
        _check(lib().hjr_scene_get_morph(self._h, C.byref(m)), "hjr_scene_get_morph")
        sets = []
        if m.n_sets:
            for s in (MorphSet * m.n_sets).from_address(m.sets):
                shape = (s.n_targets, s.n_vertices, 3)
                sets.append({"first_vertex": int(s.first_vertex), "first_weight": int(s.first_weight),
                             "position_deltas": _np(s.position_deltas, s.n_targets * s.n_vertices * 3, np.float32).reshape(shape),
                             "normal_deltas": _np(s.normal_deltas, s.n_targets * s.n_vertices * 3, np.float32).reshape(shape) if s.normal_deltas else None})
        return sets, (_np(m.default_weights, m.n_weights, np.float32) if m.n_weights else np.zeros(0, np.float32))

    def morph_weights(self, time):
        """hjr_scene_eval_morph_weights: float32 [n_weights] at `time`."""
        m = Morph()
        _check(lib().hjr_scene_get_morph(self._h, C.byref(m)), "hjr_scene_get_morph")
        w = np.zeros(m.n_weights, dtype=np.float32)
        _check(lib().hjr_scene_eval_morph_weights(self._h, C.c_float(time), w.ctypes.data if w.size else None, m.n_weights), "hjr_scene_eval_morph_weights")
        return w

    def arrays(self, time=None):
        """numpy copies of the SceneData columns (+ transforms at `time`) — the oracle's input in tests/bench."""
        v = self.view
        a = {
            "vertices": _np(v.vertices, v.n_vertices * 3, np.float32),
            "normals": _np(v.normals, v.n_vertices * 3, np.float32),
            "texcoords": _np(v.texcoords, v.n_vertices * 2, np.float32),
            "indices": _np(v.indices, v.n_triangles * 3, np.uint32),
            "material_ids": _np(v.material_ids, v.n_triangles, np.uint32),
            "prim_offsets": _np(v.prim_offset, v.n_instances, np.uint32),
            "geometry_index_offset": _np(v.geometry_index_offset, v.n_instances, np.uint32),
            "geometry_index_count": _np(v.geometry_index_count, v.n_instances, np.uint32),
            "instance_animation_id": _np(v.instance_animation_id, v.n_instances, np.uint32),
            "materials": _np(v.materials, v.n_materials, MATERIAL_DTYPE),
            "light_prim_ids": _np(v.light_prim_ids, v.n_lights, np.uint32),
            "light_prim_emission": _np(v.light_prim_emission, v.n_lights * 3, np.float32),
        }
        texs = []
        if v.n_textures:
            arr = (Texture * v.n_textures).from_address(v.textures)
            for t in arr:
                texs.append((_np(t.rgba8, t.width * t.height * 4, np.uint8).reshape(t.height, t.width, 4), int(t.srgb)))
        a["textures"] = texs
        if time is not None:
            a["transforms"], a["inv_transforms"] = self.transforms(time)
        return a


class Device:
    """One hjr_ctx (one per GPU / per process)."""

    def __init__(self, ordinal=0):
        self._h = C.c_void_p()
        _check(lib().hjr_create(ordinal, C.byref(self._h)), "hjr_create")

    def close(self):
        if self._h:
            lib().hjr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_scene(self, view):
        _check(lib().hjr_upload_scene(self._h, C.byref(view)), "hjr_upload_scene")

    def upload_arrays(self, a):
        """Upload from numpy arrays (keys as Scene.arrays())."""
        self._keep = {k: np.ascontiguousarray(a[k]) for k in ("vertices", "normals", "texcoords", "indices", "material_ids",
                                                              "prim_offsets", "materials", "light_prim_ids", "light_prim_emission")}
        k = self._keep
        v = SceneView()
        v.n_vertices = k["vertices"].size // 3
        v.n_triangles = k["indices"].size // 3
        v.n_instances = k["prim_offsets"].size
        v.n_materials = k["materials"].size
        v.n_lights = k["light_prim_ids"].size
        texs = a.get("textures") or []
        if texs:
            self._keep_tex = [np.ascontiguousarray(t[0], dtype=np.uint8) for t in texs]
            self._keep_texarr = (Texture * len(texs))()
            for i, (t, px) in enumerate(zip(texs, self._keep_tex)):
                self._keep_texarr[i].rgba8 = px.ctypes.data
                self._keep_texarr[i].height, self._keep_texarr[i].width = px.shape[0], px.shape[1]
                self._keep_texarr[i].srgb = int(t[1])
            v.n_textures = len(texs)
            v.textures = C.addressof(self._keep_texarr)
        for name, key in (("vertices", "vertices"), ("normals", "normals"), ("texcoords", "texcoords"), ("indices", "indices"),
                          ("material_ids", "material_ids"), ("prim_offset", "prim_offsets"), ("materials", "materials"),
                          ("light_prim_ids", "light_prim_ids"), ("light_prim_emission", "light_prim_emission")):
            setattr(v, name, k[key].ctypes.data if k[key].size else None)
        self.upload_scene(v)

    def set_transforms(self, m, inv):
        m = np.ascontiguousarray(m, dtype=np.float32)
        inv = np.ascontiguousarray(inv, dtype=np.float32)
        _check(lib().hjr_set_transforms(self._h, m.ctypes.data, inv.ctypes.data, m.size // 12), "hjr_set_transforms")

    def set_lut(self, rgba):
        if rgba is None:
            _check(lib().hjr_set_lut(self._h, None, 0, 0), "hjr_set_lut")
            return
        a = np.ascontiguousarray(rgba, dtype=np.uint8)
        _check(lib().hjr_set_lut(self._h, a.ctypes.data, a.shape[1], a.shape[0]), "hjr_set_lut")

    def set_sky(self, rgba32f):
        """Equirect IBL (float RGBA [h, w, 4]); None restores the constant scene_sky_default sky."""
        if rgba32f is None:
            _check(lib().hjr_set_sky(self._h, None, 0, 0), "hjr_set_sky")
            return
        a = np.ascontiguousarray(rgba32f, dtype=np.float32)
        _check(lib().hjr_set_sky(self._h, a.ctypes.data, a.shape[1], a.shape[0]), "hjr_set_sky")

    def update_vertices(self, first_vertex, positions, normals=None):
        """hjr_update_vertices: overwrite base positions (float32 [n, 3]) from `first_vertex` on, and the normals unless None."""
        p = np.ascontiguousarray(positions, dtype=np.float32)
        nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32)
        if nrm is not None and nrm.size != p.size:
            raise ValueError("update_vertices: positions and normals must have the same size")
        _check(lib().hjr_update_vertices(self._h, int(first_vertex), p.size // 3, p.ctypes.data if p.size else None,
                                         None if nrm is None else nrm.ctypes.data), "hjr_update_vertices")

    def set_morph(self, sets, default_weights=None):
        """hjr_set_morph.  sets: dicts with first_vertex, first_weight, position_deltas (float32 [K, n, 3], target-major) and optionally
        normal_deltas (the same shape); None or an empty list removes the morph.  default_weights: float32 [n_weights] (None: zeros, as many as the
        sets use)."""
        if not sets:
            _check(lib().hjr_set_morph(self._h, None), "hjr_set_morph")
            return
        keep, arr = [], (MorphSet * len(sets))()
        need = 0
        for i, s in enumerate(sets):
            pd = np.ascontiguousarray(s["position_deltas"], dtype=np.float32)
            if pd.ndim != 3 or pd.shape[2] != 3:
                raise ValueError("set_morph: position_deltas must be [targets, vertices, 3]")
            nd = s.get("normal_deltas")
            if nd is not None:
                nd = np.ascontiguousarray(nd, dtype=np.float32)
                if nd.shape != pd.shape:
                    raise ValueError("set_morph: normal_deltas must have the shape of position_deltas")
            keep += [pd, nd]
            arr[i].first_vertex, arr[i].n_vertices, arr[i].n_targets = int(s["first_vertex"]), pd.shape[1], pd.shape[0]
            arr[i].first_weight = int(s.get("first_weight", 0))
            arr[i].position_deltas = pd.ctypes.data
            arr[i].normal_deltas = None if nd is None else nd.ctypes.data
            need = max(need, arr[i].first_weight + pd.shape[0])
        m = Morph()
        m.n_sets = len(sets)
        m.sets = C.addressof(arr)
        w = None if default_weights is None else np.ascontiguousarray(default_weights, dtype=np.float32)
        m.n_weights = w.size if w is not None else need
        m.default_weights = None if w is None else w.ctypes.data
        _check(lib().hjr_set_morph(self._h, C.byref(m)), "hjr_set_morph")

    def set_morph_weights(self, weights):
        """hjr_set_morph_weights: float32 [n_weights]."""
        w = np.ascontiguousarray(weights, dtype=np.float32)
        _check(lib().hjr_set_morph_weights(self._h, w.ctypes.data if w.size else None, w.size), "hjr_set_morph_weights")

    def render(self, params, want_aovs=True, want_variance=False):
        """Synchronous render into host arrays (hjr_render); want_variance: hjr_render_var, and the variance AOV (float32 [h, w]) is
        returned as a fourth array.  With a render window (params.window) the arrays have the window's shape."""
        shp = window_shape(params) + (4,)
        color = np.zeros(shp, dtype=np.float32)
        albedo = np.zeros(shp, dtype=np.float32) if want_aovs else None
        normal = np.zeros(shp, dtype=np.float32) if want_aovs else None
        if want_variance:
            variance = np.zeros(shp[:2], dtype=np.float32)
            _check(lib().hjr_render_var(self._h, C.byref(params), color.ctypes.data, albedo.ctypes.data if want_aovs else None,
                                        normal.ctypes.data if want_aovs else None, variance.ctypes.data), "hjr_render_var")
            return color, albedo, normal, variance
        _check(lib().hjr_render(self._h, C.byref(params), color.ctypes.data,
                                albedo.ctypes.data if want_aovs else None, normal.ctypes.data if want_aovs else None), "hjr_render")
        return color, albedo, normal

    def render_progressive(self, params, passes, want_aovs=True, want_variance=False):
        """Renders the frame of `params` in `passes` sample passes (hjr_params.sample_begin / sample_end, split by pass_bounds) and yields
        (sample_end, color, albedo, normal) after each: the running mean over samples [0, sample_end).  The last one is the one-shot frame,
        bit for bit.  `params` itself is not modified.  want_variance: the variance AOV of each pass is yielded as a fifth item."""
        for begin, end in pass_bounds(params.spp, passes):
            p = ParamsV3()
            C.memmove(C.addressof(p), C.addressof(params), min(C.sizeof(params), C.sizeof(p)))
            p.struct_size = C.sizeof(p)
            p.sample_begin, p.sample_end = begin, end
            yield (end,) + tuple(self.render(p, want_aovs, want_variance))

    def set_adaptive(self, noise_threshold, min_samples=0):
        """hjr_set_adaptive: converged 8x8 tiles stop between the sample passes of a frame (mean relative error of the tile's pixels at
        most noise_threshold; no decision before min_samples, 0 = two granules).  0 switches it off.  Ends an unfinished progressive frame."""
        a = Adaptive()
        a.noise_threshold, a.min_samples = noise_threshold, min_samples
        _check(lib().hjr_set_adaptive(self._h, C.byref(a)), "hjr_set_adaptive")

    def adaptive_state(self):
        """hjr_get_adaptive_state as a dict: owned_tiles, active_tiles, sample_end, samples_rendered (synchronous)."""
        s = AdaptiveState()
        _check(lib().hjr_get_adaptive_state(self._h, C.byref(s)), "hjr_get_adaptive_state")
        return {n: int(getattr(s, n)) for n, _ in AdaptiveState._fields_ if n != "struct_size"}

    def tile_samples(self):
        """hjr_copy_tile_samples: uint32 [owned tiles], the samples each owned tile of the adaptive frame has received."""
        out = np.zeros(self.adaptive_state()["owned_tiles"], dtype=np.uint32)
        _check(lib().hjr_copy_tile_samples(self._h, out.ctypes.data, out.size), "hjr_copy_tile_samples")
        return out

    def render_adaptive(self, params, passes, want_aovs=True, want_variance=False):
        """render_progressive for a context with set_adaptive on: yields (sample_end, color, albedo, normal) after each pass and ends with
        the first pass that leaves no tile active (or at spp); the last AOVs yielded are the frame."""
        for out in self.render_progressive(params, passes, want_aovs, want_variance):
            yield out
            if out[0] < params.spp and self.adaptive_state()["active_tiles"] == 0:
                return

    def render_device(self, params, d_color, d_albedo=None, d_normal=None, stream=None, d_variance=None):
        """Asynchronous render into device pointers (ints, e.g. torch tensor .data_ptr()) on a hipStream_t (int); d_variance: one float
        per pixel (hjr_render_device_var)."""
        if d_variance:
            _check(lib().hjr_render_device_var(self._h, C.byref(params), C.c_void_p(d_color), C.c_void_p(d_albedo) if d_albedo else None,
                                               C.c_void_p(d_normal) if d_normal else None, C.c_void_p(d_variance),
                                               C.c_void_p(stream) if stream else None), "hjr_render_device_var")
            return
        _check(lib().hjr_render_device(self._h, C.byref(params), C.c_void_p(d_color),
                                       C.c_void_p(d_albedo) if d_albedo else None, C.c_void_p(d_normal) if d_normal else None,
                                       C.c_void_p(stream) if stream else None), "hjr_render_device")

    def blit_window_device(self, d_window, window, d_frame, width, height, stream=None):
        """hjr_blit_window_device: the float4 image of a window launch (device pointer, ints as in render_device) into rows y0 .. y1 - 1,
        columns x0 .. x1 - 1 of a width x height float4 frame on the device; asynchronous on `stream`."""
        w = (C.c_uint32 * 4)(*window)
        _check(lib().hjr_blit_window_device(self._h, C.c_void_p(d_window), w, C.c_void_p(d_frame), width, height,
                                            C.c_void_p(stream) if stream else None), "hjr_blit_window_device")

    def denoise(self, mode, color, albedo=None, normal=None, variance=None):
        """OptixDenoiserManager::denoise() replacement on host float4 images (hjr_denoise); returns AOV_Output.  With `variance`
        (float32 [h, w], the variance AOV) the variance-guided filter runs instead (hjr_denoise_var)."""
        color = np.ascontiguousarray(color, dtype=np.float32)
        h, w = color.shape[:2]
        ow, oh = (2 * w, 2 * h) if mode == MODE_DENOISE_UPSCALE2X else (w, h)
        a = None if albedo is None else np.ascontiguousarray(albedo, dtype=np.float32)
        n = None if normal is None else np.ascontiguousarray(normal, dtype=np.float32)
        out = np.zeros((oh, ow, 4), dtype=np.float32)
        if variance is not None:
            v = np.ascontiguousarray(variance, dtype=np.float32)
            if v.shape != (h, w):
                raise ValueError("variance must be [height, width]")
            _check(lib().hjr_denoise_var(self._h, mode, w, h, color.ctypes.data, None if a is None else a.ctypes.data,
                                         None if n is None else n.ctypes.data, v.ctypes.data, out.ctypes.data, ow, oh), "hjr_denoise_var")
            return out
        _check(lib().hjr_denoise(self._h, mode, w, h, color.ctypes.data, None if a is None else a.ctypes.data,
                                 None if n is None else n.ctypes.data, out.ctypes.data, ow, oh), "hjr_denoise")
        return out

    def estimate_variance(self, color, albedo, normal, variance=None):
        """hjr_estimate_variance on host float4 images [h, w, 4]: pixels of `variance` (float32 [h, w]; None = all of them) that are unknown
        (VARIANCE_UNKNOWN or above) get the 3 x 3 guide-weighted variance of r + g + b, the others keep their bits.  Returns float32 [h, w]."""
        color, albedo, normal = (np.ascontiguousarray(a, dtype=np.float32) for a in (color, albedo, normal))
        h, w = color.shape[:2]
        if color.shape != (h, w, 4) or albedo.shape != (h, w, 4) or normal.shape != (h, w, 4):
            raise ValueError("color, albedo and normal must be [height, width, 4]")
        v = None
        if variance is not None:
            v = np.ascontiguousarray(variance, dtype=np.float32)
            if v.shape != (h, w):
                raise ValueError("variance must be [height, width]")
        out = np.zeros((h, w), dtype=np.float32)
        _check(lib().hjr_estimate_variance(self._h, w, h, color.ctypes.data, albedo.ctypes.data, normal.ctypes.data, None if v is None else v.ctypes.data,
                                           out.ctypes.data), "hjr_estimate_variance")
        return out

    def estimate_variance_device(self, width, height, d_color, d_albedo, d_normal, d_variance_in, d_variance_out, stream=None):
        """hjr_estimate_variance_device: the same on device pointers (ints; d_variance_in None = every pixel unknown; d_variance_out may be
        d_variance_in), asynchronous on a hipStream_t (int; None = the context's stream)."""
        _check(lib().hjr_estimate_variance_device(self._h, width, height, C.c_void_p(d_color), C.c_void_p(d_albedo), C.c_void_p(d_normal),
                                                  C.c_void_p(d_variance_in) if d_variance_in else None, C.c_void_p(d_variance_out),
                                                  C.c_void_p(stream) if stream else None), "hjr_estimate_variance_device")

    def render_denoised(self, params, mode, out_w=None, out_h=None):
        """One frame in a render mode, AOVs kept on the device (hjr_render_denoised); returns AOV_Output."""
        ow = out_w if out_w is not None else (2 * params.width if mode == MODE_DENOISE_UPSCALE2X else params.width)
        oh = out_h if out_h is not None else (2 * params.height if mode == MODE_DENOISE_UPSCALE2X else params.height)
        out = np.zeros((oh, ow, 4), dtype=np.float32)
        _check(lib().hjr_render_denoised(self._h, C.byref(params), mode, out.ctypes.data, ow, oh), "hjr_render_denoised")
        return out

    def assemble_shards_device(self, shards, width, height, d_color=None, d_albedo=None, d_normal=None, d_variance=None, stream=None):
        """hjr_assemble_shards_device: one launch scatters the gathered blocks of every rank and AOV of `shards` (a Shards of device
        pointers) into row-major frames at the device pointers given (ints; None for an AOV the shards do not carry).  Asynchronous."""
        _check(lib().hjr_assemble_shards_device(self._h, C.byref(shards), width, height, *[C.c_void_p(d) if d else None for d in (d_color, d_albedo, d_normal, d_variance)],
                                                C.c_void_p(stream) if stream else None), "hjr_assemble_shards_device")

    def denoise_shards(self, params, mode, shards, out_w=None, out_h=None):
        """Rank 0's half of a multi-GPU frame in a Denoise mode (hjr_denoise_shards_device): `shards` (a Shards of device pointers) are
        assembled and go through what render_denoised runs after its render, under the same context options; `params` describes the whole
        frame at the render size.  Runs on the context's stream; returns AOV_Output as numpy."""
        import torch
        ow = out_w if out_w is not None else (2 * params.width if mode == MODE_DENOISE_UPSCALE2X else params.width)
        oh = out_h if out_h is not None else (2 * params.height if mode == MODE_DENOISE_UPSCALE2X else params.height)
        out = torch.empty((max(oh, 1), max(ow, 1), 4), dtype=torch.float32, device="cuda")
        _check(lib().hjr_denoise_shards_device(self._h, C.byref(params), mode, C.byref(shards), C.c_void_p(out.data_ptr()), ow, oh, None), "hjr_denoise_shards_device")
        self.synchronize()
        return out[:oh, :ow].cpu().numpy()

    def gbuffer(self, params, coverage=0):
        """hjr_render_gbuffer: the first hit of every pixel's centre ray against the current frame data, GBUFFER_DTYPE [height, width]
        (width, height and camera of `params` are read).  coverage 2, 3 or 4: hjr_render_gbuffer_cov with that side, the same records
        with pad = same | (side * side) << 8."""
        out = np.zeros((params.height, params.width), dtype=GBUFFER_DTYPE)
        if coverage:
            _check(lib().hjr_render_gbuffer_cov(self._h, C.byref(params), coverage, out.ctypes.data), "hjr_render_gbuffer_cov")
        else:
            _check(lib().hjr_render_gbuffer(self._h, C.byref(params), out.ctypes.data), "hjr_render_gbuffer")
        return out

    @staticmethod
    def _temporal_frame(d, keep, images=True):
        """dict -> TemporalFrame: camera (Camera or dict), transforms / inv_transforms [n, 12], gbuffer (GBUFFER_DTYPE [h, w]), color
        [h, w, 4], variance [h, w] and, for the previous frame, history [h, w]; optional coverage (non-zero: the G-buffer's pad words are
        coverage counts)."""
        g = np.ascontiguousarray(d["gbuffer"], dtype=GBUFFER_DTYPE)
        h, w = g.shape
        m = np.ascontiguousarray(d["transforms"], dtype=np.float32).reshape(-1, 12)
        inv = np.ascontiguousarray(d["inv_transforms"], dtype=np.float32).reshape(-1, 12)
        col = np.ascontiguousarray(d["color"], dtype=np.float32) if images else None
        var = np.ascontiguousarray(d["variance"], dtype=np.float32) if images else None
        if m.shape != inv.shape or (images and (col.shape != (h, w, 4) or var.shape != (h, w))):
            raise ValueError("temporal frame: array shapes do not agree")
        f = TemporalFrame()
        f.width, f.height, f.n_instances = w, h, m.shape[0]
        cam = d["camera"]
        f.camera = cam if isinstance(cam, Camera) else make_params(w, h, 1, cam).camera
        arrs = [m, inv, g, col, var]
        f.transforms12, f.inv_transforms12 = m.ctypes.data if m.size else None, inv.ctypes.data if inv.size else None
        f.gbuffer, f.color, f.variance = g.ctypes.data, col.ctypes.data if images else None, var.ctypes.data if images else None
        f.coverage = int(d.get("coverage") or 0)
        if d.get("history") is not None:
            hist = np.ascontiguousarray(d["history"], dtype=np.float32)
            if hist.shape != (h, w):
                raise ValueError("temporal frame: history must be [height, width]")
            f.history = hist.ctypes.data
            arrs.append(hist)
        keep.append(arrs)
        return f

    def temporal_accumulate(self, prev, cur, moments=False, response=False):
        """hjr_temporal_accumulate on dicts of arrays (keys: camera, transforms, inv_transforms, gbuffer, color, variance, optionally coverage; prev also
        history; prev None = no previous frame): returns (color [h, w, 4], variance [h, w], history [h, w]).  moments=True:
        hjr_temporal_accumulate_moments, which reads prev["moments"] ([h, w, 2], passed as its prev_moments argument) and returns a fourth
        array, the moments [h, w, 2].  response=True: hjr_temporal_accumulate_response, with or without the moments, which returns lambda
        [h, w] as a further array (the last one)."""
        keep = []
        fc = self._temporal_frame(cur, keep)
        fp = None if prev is None else self._temporal_frame(prev, keep)
        h, w = fc.height, fc.width
        color = np.zeros((h, w, 4), dtype=np.float32)
        variance = np.zeros((h, w), dtype=np.float32)
        history = np.zeros((h, w), dtype=np.float32)
        if moments or response:
            mom = np.zeros((h, w, 2), dtype=np.float32) if moments else None
            pm = None
            if moments and prev is not None and prev.get("moments") is not None:
                pm = np.ascontiguousarray(prev["moments"], dtype=np.float32)
                if pm.shape != (h, w, 2):
                    raise ValueError("temporal frame: moments must be [height, width, 2]")
            if response:
                lam = np.zeros((h, w), dtype=np.float32)
                _check(lib().hjr_temporal_accumulate_response(self._h, None if fp is None else C.byref(fp), C.byref(fc), color.ctypes.data, variance.ctypes.data,
                                                              history.ctypes.data, None if pm is None else pm.ctypes.data, None if mom is None else mom.ctypes.data,
                                                              lam.ctypes.data), "hjr_temporal_accumulate_response")
                return (color, variance, history, mom, lam) if moments else (color, variance, history, lam)
            _check(lib().hjr_temporal_accumulate_moments(self._h, None if fp is None else C.byref(fp), C.byref(fc), color.ctypes.data, variance.ctypes.data,
                                                         history.ctypes.data, None if pm is None else pm.ctypes.data, mom.ctypes.data),
                   "hjr_temporal_accumulate_moments")
            return color, variance, history, mom
        _check(lib().hjr_temporal_accumulate(self._h, None if fp is None else C.byref(fp), C.byref(fc), color.ctypes.data, variance.ctypes.data,
                                             history.ctypes.data), "hjr_temporal_accumulate")
        return color, variance, history

    def temporal_prior(self, prev, cur):
        """hjr_temporal_prior on dicts of arrays as temporal_accumulate takes them (prev None = no previous frame); cur needs camera,
        transforms, inv_transforms, gbuffer and optionally coverage only: its colour and variance are not read.  Returns the prior
        [h, w, 4]: (lp, vp, al, 0) per pixel, (0, 0, 1, 0) where the history contributes nothing (adaptive sampling's rule 11)."""
        keep = []
        fc = self._temporal_frame(cur, keep, images=False)
        fp = None if prev is None else self._temporal_frame(prev, keep)
        prior = np.zeros((fc.height, fc.width, 4), dtype=np.float32)
        _check(lib().hjr_temporal_prior(self._h, None if fp is None else C.byref(fp), C.byref(fc), prior.ctypes.data), "hjr_temporal_prior")
        return prior

    def upscale_guided(self, color_lo, gbuffer_lo, cam, gbuffer_hi):
        """hjr_upscale_guided on host arrays: color_lo float32 [h, w, 4] (the filtered half-size image), gbuffer_lo GBUFFER_DTYPE [h, w],
        gbuffer_hi GBUFFER_DTYPE [oh, ow] with ow // 2 == w and oh // 2 == h (Device.gbuffer at both sizes from `cam`, a Camera or dict).
        Returns float32 [oh, ow, 4]."""
        color_lo = np.ascontiguousarray(color_lo, dtype=np.float32)
        lo = np.ascontiguousarray(gbuffer_lo, dtype=GBUFFER_DTYPE)
        hi = np.ascontiguousarray(gbuffer_hi, dtype=GBUFFER_DTYPE)
        h, w = lo.shape
        oh, ow = hi.shape
        if color_lo.shape != (h, w, 4):
            raise ValueError("color_lo must be [height, width, 4] of gbuffer_lo's size")
        c = cam if isinstance(cam, Camera) else make_params(w, h, 1, cam).camera
        out = np.zeros((oh, ow, 4), dtype=np.float32)
        _check(lib().hjr_upscale_guided(self._h, w, h, color_lo.ctypes.data, lo.ctypes.data, C.byref(c), hi.ctypes.data, out.ctypes.data, ow, oh),
               "hjr_upscale_guided")
        return out

    def upscale_guided_device(self, width, height, d_color_lo, d_gbuffer_lo, cam, d_gbuffer_hi, d_out, out_w, out_h, stream=None):
        """hjr_upscale_guided_device: the same on device pointers (ints), one launch, asynchronous on a hipStream_t (int; None = the
        context's stream); `cam` is a Camera or dict, read during the call."""
        c = cam if isinstance(cam, Camera) else make_params(width, height, 1, cam).camera
        _check(lib().hjr_upscale_guided_device(self._h, width, height, C.c_void_p(d_color_lo), C.c_void_p(d_gbuffer_lo), C.byref(c), C.c_void_p(d_gbuffer_hi),
                                               C.c_void_p(d_out), out_w, out_h, C.c_void_p(stream) if stream else None), "hjr_upscale_guided_device")

    def temporal_reset(self):
        """hjr_temporal_reset: drops the history of option "denoise_temporal"; the next frame restarts everywhere."""
        _check(lib().hjr_temporal_reset(self._h), "hjr_temporal_reset")

    def synchronize(self):
        _check(lib().hjr_synchronize(self._h), "hjr_synchronize")

    def preview_device(self, d_color, width, height, tonemap, d_rgba8, stream=None):
        """hjr_preview_device: the raygen's 8-bit preview image from a float4 colour image, device pointers (ints)."""
        _check(lib().hjr_preview_device(self._h, C.c_void_p(d_color), width, height, tonemap, C.c_void_p(d_rgba8),
                                        C.c_void_p(stream) if stream else None), "hjr_preview_device")

    def set_option(self, key, value):
        """hjr_set_option: tuning / test option of this context (-1 restores the default); layout options act at the next set_transforms.
        "firefly_clamp" (kappa, 0..64) clamps whole-frame renders; with "firefly_clamp_passes" 1 next to it sample passes and adaptive
        frames are accepted and clamped too (the colour chunk sums of the whole progressive frame are kept; include/henjou_hip.h "Firefly
        clamp on sample passes").  Setting "firefly_clamp_passes", or "firefly_clamp" while it is 1, ends an unfinished progressive frame.
        "adaptive_temporal" 1 lets the sample passes of render_denoised on an adaptive frame with "denoise_temporal" on stop a tile on the
        error of the accumulated pixel (rule 11) and commits the history when the last tile stops; setting it ends an unfinished
        progressive frame too."""
        _check(lib().hjr_set_option(self._h, key.encode(), int(value)), "hjr_set_option")

    def get_option(self, key):
        v = C.c_int()
        _check(lib().hjr_get_option(self._h, key.encode(), C.byref(v)), "hjr_get_option")
        return v.value

    def copy_frame_data(self, what):
        """hjr_copy_frame_data: the current frame data as float32 [records, 4] (what = FRAME_NODES / FRAME_TRI_GEOM / FRAME_TRI_SHADE /
        FRAME_LIGHTS; layouts in csrc/hjr_layout.h; child refs and ids are uint32 bits: .view(np.uint32))."""
        n = C.c_size_t()
        _check(lib().hjr_copy_frame_data(self._h, what, None, 0, C.byref(n)), "hjr_copy_frame_data")
        out = np.zeros(n.value // 4, dtype=np.float32)
        if n.value:
            _check(lib().hjr_copy_frame_data(self._h, what, out.ctypes.data, n.value, C.byref(n)), "hjr_copy_frame_data")
        return out.reshape(-1, 4)

    def trace_rays(self, path, shadow, closest):
        """hjr_trace_rays (test hook): arrays of RAY_DTYPE, pair i = (shadow[i], closest[i]) -> array of RAY_RESULT_DTYPE.
        path = TRACE_STANDALONE / TRACE_FUSED, optionally | TRACE_FAST_BUILD."""
        shadow = np.ascontiguousarray(shadow, dtype=RAY_DTYPE)
        closest = np.ascontiguousarray(closest, dtype=RAY_DTYPE)
        if shadow.shape != closest.shape or shadow.ndim != 1:
            raise ValueError("trace_rays: shadow and closest must be 1-D arrays of the same length")
        out = np.zeros(shadow.size, dtype=RAY_RESULT_DTYPE)
        _check(lib().hjr_trace_rays(self._h, int(path), shadow.size, shadow.ctypes.data if shadow.size else None,
                                    closest.ctypes.data if shadow.size else None, out.ctypes.data if shadow.size else None), "hjr_trace_rays")
        return out

    def stats(self):
        st = StatsV7()
        _check(lib().hjr_get_stats(self._h, C.byref(st)), "hjr_get_stats")
        return st.as_dict()


def make_params(width, height, spp, camera, frame=1, seed=1, integrator=INTEGRATOR_NEE, sky=(0.8, 0.8, 0.8),
                ibl_intensity=1.0, rank=0, world_size=1, flags=0, sample_begin=0, sample_end=0, window=None):
    """hjr_params.  window: (x0, y0, x1, y1), the render window in full-frame pixels: a ParamsV3.  None = the whole frame, as the ParamsV2
    this function always returned (the shorter caller of the sized-struct rule)."""
    p = ParamsV2() if window is None else ParamsV3()
    p.width, p.height, p.spp, p.frame, p.seed, p.integrator = width, height, spp, frame, seed, integrator
    if isinstance(camera, Camera):
        p.camera = camera
    else:
        p.camera.pos = (C.c_float * 3)(*camera["pos"])
        p.camera.dir = (C.c_float * 3)(*camera["dir"])
        p.camera.up = (C.c_float * 3)(*camera["up"])
        p.camera.right = (C.c_float * 3)(*camera["right"])
        p.camera.f = camera["f"]
    p.sky = (C.c_float * 3)(*sky)
    p.ibl_intensity = ibl_intensity
    p.rank, p.world_size, p.flags = rank, world_size, flags
    p.sample_begin, p.sample_end = sample_begin, sample_end
    if window is not None:
        p.window = (C.c_uint32 * 4)(*window)
    return p


def window_shape(params):
    """(rows, columns) of the outputs of a launch with `params`: the window's, or else the frame's (a caller without the field: the frame's)."""
    win = getattr(params, "window", None)
    if win is not None and win[2] != 0:
        return (int(win[3]) - int(win[1]), int(win[2]) - int(win[0]))
    return (params.height, params.width)


def bucket_windows(width, height, bw, bh):
    """The buckets of a width x height frame as windows [(x0, y0, x1, y1), ...]: bw x bh rectangles (multiples of 8), row-major from (0, 0),
    edge buckets clipped to the frame (hjr_bucket_count / hjr_bucket_window)."""
    n = int(lib().hjr_bucket_count(width, height, bw, bh))
    if n == 0:
        raise HjrError("bucket_windows: the frame must not be empty and the bucket sides must be positive multiples of 8")
    out = []
    for i in range(n):
        w = (C.c_uint32 * 4)()
        _check(lib().hjr_bucket_window(width, height, bw, bh, i, w), "hjr_bucket_window")
        out.append(tuple(int(v) for v in w))
    return out


def blit_window(window_rgba, window, frame):
    """hjr_blit_window: writes the float4 image of a window launch into its rectangle of `frame` (row-major float4, modified in place)."""
    a = np.ascontiguousarray(window_rgba, dtype=np.float32)
    h, w = frame.shape[:2]
    assert frame.dtype == np.float32 and frame.flags["C_CONTIGUOUS"]
    x0, y0, x1, y1 = window
    if a.shape != (y1 - y0, x1 - x0, 4):
        raise HjrError("blit_window: the image must have the window's shape")
    _check(lib().hjr_blit_window(a.ctypes.data, (C.c_uint32 * 4)(*window), frame.ctypes.data, w, h), "hjr_blit_window")
    return frame


def owned_tile_mask(width, height, rank, world_size, tile=8):
    """Boolean [height, width] mask of the pixels rank `rank` renders: 8x8 tiles, tile (tx, ty) has id ty * tiles_x + (tx + ty) % tiles_x
    (rows rotated so that a rank's tiles run along diagonals, csrc/hjr_layout.h) and belongs to rank id % world_size."""
    tx = (np.arange(width) // tile)[None, :]
    ty = (np.arange(height) // tile)[:, None]
    tiles_x = (width + tile - 1) // tile
    return ((ty * tiles_x + (tx + ty) % tiles_x) % world_size) == rank


def exchange_framebuffer(fb, dst=0):
    """Full-frame form of the multi-GPU exchange (what north_star names): every rank holds its own 8x8 tiles and zeros
    elsewhere (HJR_FLAG_ZERO_UNOWNED); a SUM reduce onto `dst` assembles the frame.  Adding zeros is exact in IEEE arithmetic,
    so the result is bit-identical to the 1-GPU image.  `fb` is a torch tensor (CUDA -> RCCL over xGMI; CPU -> gloo in the
    tests).  gather_tiles below moves 1 / world of these bytes and is what bench.py and henjou_cli use."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.reduce(fb, dst=dst, op=dist.ReduceOp.SUM)
    return fb


def sample_granule(spp):
    """hjr_sample_granule: the boundary granule of a frame's sample passes (one work-item chunk; spp itself for a single-chunk frame)."""
    return int(lib().hjr_sample_granule(spp))


def pass_bounds(spp, passes, granule=None):
    """The sample passes [(begin, end), ...] of a frame of `spp` samples split into `passes` (1..64): pass k ends at k * spp // passes rounded
    down to the granule (sample_granule(spp) unless given), the last at spp; passes that come out empty are dropped.  The same split as
    "Henjou_HIP": {"passes": N} in hjr_render_file / henjou_cli."""
    if not 1 <= passes <= 64:
        raise ValueError("passes must be in [1, 64]")
    g = sample_granule(spp) if granule is None else granule
    ends = []
    for k in range(1, passes):
        e = (k * spp // passes) // g * g if g else 0
        if e > (ends[-1] if ends else 0):
            ends.append(e)
    ends.append(spp)
    return list(zip([0] + ends[:-1], ends))


def owned_tiles(width, height, rank, world_size):
    return int(lib().hjr_owned_tiles(width, height, rank, world_size))


def pack_tiles(frame, rank, world_size):
    """Host form of the packed layout: [owned tile][64] float4 of `rank` from a row-major float4 frame (hjr_pack_tiles)."""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    h, w = frame.shape[:2]
    out = np.zeros((owned_tiles(w, h, rank, world_size), 64, 4), dtype=np.float32)
    _check(lib().hjr_pack_tiles(frame.ctypes.data, w, h, rank, world_size, out.ctypes.data), "hjr_pack_tiles")
    return out


def unpack_tiles(packed, frame, rank, world_size):
    """Scatters one rank's packed tiles into `frame` (row-major float4, modified in place; hjr_unpack_tiles)."""
    packed = np.ascontiguousarray(packed, dtype=np.float32)
    h, w = frame.shape[:2]
    assert frame.dtype == np.float32 and frame.flags["C_CONTIGUOUS"]
    _check(lib().hjr_unpack_tiles(packed.ctypes.data, w, h, rank, world_size, frame.ctypes.data), "hjr_unpack_tiles")
    return frame


def shards_layout(width, height, world_size, guides=True, variance=True):
    """The per-rank buffer of a Denoise-mode multi-GPU frame, colour | albedo | normal | variance, every AOV sized for rank 0 (which owns the
    most tiles): ({aov name: byte offset}, bytes per rank = the rank_stride of the gathered buffer)."""
    slots = owned_tiles(width, height, 0, world_size) * 64
    names = ["color"] + (["albedo", "normal"] if guides else []) + (["variance"] if variance else [])
    off, n = {}, 0
    for k in names:
        off[k] = n
        n += slots * (4 if k == "variance" else 16)
    return off, n


def make_shards(base_ptr, world_size, rank_stride, offsets):
    """Shards over one gathered buffer at address `base_ptr` (host or device), laid out per rank as shards_layout says."""
    s = Shards()
    s.world_size, s.rank_stride = world_size, rank_stride
    for k, o in offsets.items():
        setattr(s, k, base_ptr + o)
    return s


def assemble_shards(shards, width, height):
    """Host form (hjr_assemble_shards; no GPU): scatters the blocks of every rank and AOV of `shards` (a Shards of host pointers) into
    row-major frames; returns (color, albedo, normal [h, w, 4], variance [h, w]) with None for an AOV the shards do not carry."""
    outs = [np.zeros((height, width, 4), dtype=np.float32) if getattr(shards, k) else None for k in ("color", "albedo", "normal")]
    outs.append(np.zeros((height, width), dtype=np.float32) if shards.variance else None)
    _check(lib().hjr_assemble_shards(C.byref(shards), width, height, *[None if o is None else o.ctypes.data for o in outs]), "hjr_assemble_shards")
    return tuple(outs)


def gather_tiles(packed, width, height, device=None, dst=0, frame=None):
    """The multi-GPU exchange sized by ownership: every rank contributes its packed tiles
    ([max owned tiles][64][4] float32 torch tensor, the same shape on every rank: ranks owning one tile fewer pad), rank `dst`
    receives the world_size blocks (RCCL gather = point-to-point sends over xGMI, all peers in parallel) and scatters each into
    the row-major frame: on a CUDA tensor with hjr_unpack_tiles_device (`device` = the rank's hjr Device), on a CPU tensor
    (gloo, tests) with hjr_unpack_tiles.  Returns the assembled frame on `dst`, None elsewhere."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    blocks = None
    if world > 1:
        if rank == dst:
            blocks = [torch.empty_like(packed) for _ in range(world)]
        dist.gather(packed, gather_list=blocks, dst=dst)
    else:
        blocks = [packed]
    if rank != dst:
        return None
    if frame is None:
        frame = torch.zeros((height, width, 4), dtype=torch.float32, device=packed.device)
    for r, blk in enumerate(blocks):
        if blk.is_cuda:
            _check(lib().hjr_unpack_tiles_device(device._h, C.c_void_p(blk.data_ptr()), width, height, r, world, C.c_void_p(frame.data_ptr()),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hjr_unpack_tiles_device")
        else:
            unpack_tiles(blk.numpy(), frame.numpy(), r, world)
    return frame


class Renderer:
    """Mirror of the reference's `class Renderer` (renderer/renderer.h:900-1318) on top of the C-ABI."""

    def __init__(self, device_ordinal=0):
        self.device_ordinal = device_ordinal
        self.render_option = None
        self.scene = None
        self.device = None

    def loadRenderOption(self, path):  # renderer.h:1041-1051
        self.render_option = load_render_option(path)
        return True

    def setRenderOption(self, opt):  # renderer.h:992-995
        self.render_option = opt

    def loadGLTFfile(self, filepath, filename):  # renderer.h:1005-1013
        self.scene = Scene(filepath, filename, self.render_option)
        return True

    def build(self):  # renderer.h:1015-1039
        self.device = Device(self.device_ordinal)
        self.device.upload_scene(self.scene.view)
        lut_path = self.render_option.LUT_path.decode()
        self.lut = None
        if lut_path and os.path.exists(lut_path):
            self.lut = load_png(lut_path)
            self.device.set_lut(self.lut)
        ibl = self.render_option.IBL_path.decode()
        if self.render_option.use_IBL and ibl and os.path.exists(ibl):  # setSky (renderer.h:802-851)
            self.device.set_sky(load_hdr(ibl))

    def frame_params(self, frame, spp=None, rank=0, world_size=1, flags=0):
        o = self.render_option
        time = frame / float(o.fps)
        cam = self.scene.camera(o, time)
        return make_params(o.image_width, o.image_height, spp or o.max_spp, cam, frame=frame, seed=o.seed,
                           integrator=o.integrator, sky=tuple(o.scene_sky_default), ibl_intensity=o.IBL_intensity,
                           rank=rank, world_size=world_size, flags=flags), time

    def render_frame(self, frame, spp=None):
        """One iteration of the frame loop (renderer.h:1126-1245): IAS update, camera, launch; returns float4 AOVs."""
        p, time = self.frame_params(frame, spp)
        m, inv = self.scene.transforms(time)
        self.device.set_transforms(m, inv)
        return self.device.render(p)

    def initializeAndRender(self, render_option_path):  # renderer.h:1053-1317
        _check(lib().hjr_render_file(os.fsencode(render_option_path), self.device_ordinal), "hjr_render_file")
        return True
