/*
 * henjou_hip.h — C-ABI of libhenjou_hip.so, the MI355X-native replacement for Henjou-Renderer's
 * per-pixel-sample hot path (ray generation -> BVH traversal -> BSDF -> NEE integrator).
 *
 * Plain C, no exceptions across the boundary, no torch / STL types in any signature.
 * Every entry point cites the reference interface it replaces (paths relative to the reference's
 * include/ directory).  Status codes: 0 = ok, negative = error; hjr_last_error() gives the text.
 *
 * The reference's in-process boundary is
 *     cudaMemcpy(d_param, &params) ; optixLaunch(pipeline, stream, d_param, sizeof(Params), &sbt, W, H, 1)
 * (renderer/renderer.h:1229-1242) against six OptiX programs that read `Params` (kernel/Payload.h:8-10)
 * and per-material HitGroupData records (renderer/renderer.h:647-738).  Its file-level surface is
 * render_option.json + a glTF scene in, <image_name>_<frame>.png out (renderer/renderer.h:1053-1317).
 * Both levels are exported here.
 */
#ifndef HENJOU_HIP_H
#define HENJOU_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HJR_OK 0
#define HJR_ERR_ARG (-1)     /* bad argument / null pointer / size mismatch */
#define HJR_ERR_IO (-2)      /* file missing or unreadable */
#define HJR_ERR_PARSE (-3)   /* malformed JSON / glTF / PNG, or a mandatory key is absent */
#define HJR_ERR_DEVICE (-4)  /* HIP runtime error, or no gfx950 device / kernel image */
#define HJR_ERR_STATE (-5)   /* call order violated (render before upload, ...) */

/* ---- Sized structs (the rule that keeps callers and library binary-compatible across releases) --------------------------------
 * hjr_scene_view, hjr_render_option, hjr_params, hjr_stats, hjr_adaptive, hjr_adaptive_state, hjr_shards and hjr_morph may GROW at their end in later releases.  Each starts with
 * `struct_size`: the CALLER sets it to sizeof(its own struct) before handing the struct to ANY entry point, input or output
 * (HJR_INIT does it together with the zero fill).  The library copies min(struct_size, its own sizeof) bytes in either direction:
 *   - a field the caller's (older, shorter) struct does not have is never written and reads as 0, which selects the default;
 *   - a field a newer caller has and this library does not know is left untouched on output and ignored on input;
 *   - struct_size == 0 (a struct that was zero-filled but not initialised) is rejected with HJR_ERR_ARG.
 * The reference passes its launch block the same way: optixLaunch(..., d_param, sizeof(Params), ...) (renderer/renderer.h:1241).
 * hjr_material, hjr_texture and hjr_camera are array elements / embedded records of fixed layout (reserved words inside). */
#define HJR_INIT(s) do { memset(&(s), 0, sizeof(s)); (s).struct_size = (uint32_t)sizeof(s); } while (0) /* needs <string.h> */

enum { HJR_INTEGRATOR_NEE = 0, HJR_INTEGRATOR_PT = 1, HJR_INTEGRATOR_MIS = 2 }; /* kernel/rt.h:162,85,284 */
enum { HJR_MODE_DEFAULT = 0, HJR_MODE_DENOISE = 1, HJR_MODE_DENOISE_UPSCALE2X = 2, HJR_MODE_DEBUG = 3 }; /* renderer/render_option.h:38-43 */

/* Material record of the hot path: the fields of HitGroupData (renderer/renderer.h:659-687, filled from Material,
 * renderer/material.h:10-63) that the kernel-side code under include/kernel/ reads, in a 16-byte-aligned 80-byte layout.
 * It is NOT field-for-field HitGroupData; a binding fills it per material like this (INTEGRATION.md has the code):
 *   kept as is : basecolor, metallic, roughness, sheen, clearcoat, ior, transmission, emmision -> emission, is_light,
 *                ideal_specular, is_thinfilm, basecolor_tex, normal_tex, emmision_tex -> emission_tex
 *   merged     : metallic_tex + roughness_tex -> metallic_roughness_tex (the glTF loader always binds the same image to both,
 *                gltfloader.h:1144-1156; G = roughness, B = metallic)
 *   dropped    : specular (float3; no kernel header reads it), clearcoat_tex, bump_tex (bound by the host, read only by the
 *                missing closest-hit program; the clearcoat factor itself is kept)
 * normal_tex is sampled (tangent-space normal map, build-defined frame: DESIGN.md §10); emission_tex is always -1 on the glTF path. */
typedef struct hjr_material {
    float basecolor[3];
    float metallic;
    float roughness;
    float sheen;
    float clearcoat;
    float ior;
    float transmission;
    float emission[3];
    int32_t is_light;
    int32_t ideal_specular;
    int32_t is_thinfilm;
    int32_t basecolor_tex;   /* texture slot or -1 (Material.base_color_tex, TexType::sRGB, gltfloader.h:1133-1140) */
    int32_t metallic_roughness_tex; /* slot or -1 (metallic_tex == roughness_tex, NonColor, gltfloader.h:1144-1156): G = roughness, B = metallic */
    int32_t normal_tex;      /* slot or -1 (Material.normal_tex, NonColor, gltfloader.h:1168-1175): tangent-space normal map, per-triangle tangent frame (build-defined) */
    int32_t emission_tex;    /* always -1 on the glTF path (gltfloader.h:1159) */
    int32_t _reserved;
} hjr_material;              /* 80 bytes */

/* Texture(filename, type) — renderer/texture.h:16-39: 8-bit RGBA, bound wrap + linear + normalised coords, sRGB decode
 * unless NonColor (renderer.h:740-800). */
typedef struct hjr_texture {
    const uint8_t* rgba8;    /* width * height * 4, row 0 = top image row */
    uint32_t width, height;
    int32_t srgb;            /* 1: TexType::sRGB, 0: NonColor */
    int32_t _reserved;
} hjr_texture;

/* Borrowed, read-only view of SceneData (renderer/scene.h:19-36).  The library copies on upload. */
typedef struct hjr_scene_view {
    uint32_t struct_size;    /* sizeof(hjr_scene_view) of the caller (HJR_INIT) */
    uint32_t n_vertices;     /* == 3 * n_triangles on the glTF path (de-indexed, gltfloader.h:1484-1492) */
    uint32_t n_triangles;
    uint32_t n_instances;    /* instance i <-> geometry i, 1:1 (gltfloader.h:1507-1512) */
    uint32_t n_materials;
    uint32_t n_lights;       /* emissive triangles (gltfloader.h:1496-1500) */
    uint32_t n_animations;   /* == number of glTF nodes */
    uint32_t n_textures;     /* SceneData.textures (de-duplicated by file name, texture_load.h:7-20) */
    const float*    vertices;            /* float3 x n_vertices, object space */
    const float*    normals;             /* float3 x n_vertices */
    const float*    texcoords;           /* float2 x n_vertices */
    const uint32_t* indices;             /* 3 x n_triangles */
    const uint32_t* material_ids;        /* n_triangles */
    const uint32_t* prim_offset;         /* n_instances: first global triangle of the instance */
    const uint32_t* geometry_index_offset; /* n_instances (GeometryData.index_offset, scene.h:9-12) */
    const uint32_t* geometry_index_count;  /* n_instances */
    const uint32_t* instance_animation_id; /* n_instances (InstanceData.animation_id, scene.h:14-17) */
    const hjr_material* materials;
    const uint32_t* light_prim_ids;      /* n_lights, global triangle ids */
    const float*    light_prim_emission; /* float3 x n_lights */
    const hjr_texture* textures;         /* n_textures */
} hjr_scene_view;

/* Mirror of RenderOption (renderer/render_option.h:45-84). */
typedef struct hjr_render_option {
    uint32_t struct_size;        /* sizeof(hjr_render_option) of the caller (HJR_INIT) */
    uint32_t image_width, image_height;
    char image_name[256];
    char image_directory[512];
    uint32_t max_spp;
    char gltf_path[512];
    char gltf_name[256];
    uint32_t fps, start_frame, end_frame;
    float time_limit;
    int32_t allow_camera_animation;
    float camera_fov;            /* radians after load (render_json_loader.h:144) */
    float camera_position[3];
    float camera_direction[3];
    int32_t camera_animation_id; /* -1 = none */
    int32_t render_mode;         /* HJR_MODE_* */
    char ptxfile_path[512];      /* parsed, unused */
    int32_t use_IBL;
    char IBL_path[512];
    float IBL_intensity;
    float scene_sky_default[3];
    int32_t use_date, save_renderOption;
    char LUT_path[512];
    /* optional "Henjou_HIP" section (ignored by the reference): */
    uint32_t seed;               /* default 1 */
    int32_t integrator;          /* default HJR_INTEGRATOR_NEE */
    uint32_t devices;            /* default 1: GPUs of the node that share each frame (pixel-tile shard, one process per GPU) */
    uint32_t tile;               /* shard granularity in pixels; 8 is the only supported value */
    int32_t serial_io;           /* default 0; 1: hjr_render_file renders, writes and prepares the next frame one after the other (no overlap) */
    int32_t fast_math;           /* default 0; 1: hjr_render_file / henjou_cli launch with HJR_FLAG_FAST_MATH */
    /* The next three fields and denoise_variance hold thirteen keys of the section between them.  This is the whole layout; the table
     * in henjou-renderer_amd/host/render_job.hpp is its code, the one place that packs and unpacks it.  A key sets the context option of
     * its name (hjr_set_option) in hjr_render_file and henjou_cli, on the processes listed at the end of the hjr_set_option comment. */
    int32_t force_rebuild;       /* default 0; bit 0: key "force_rebuild" (the frame data is rebuilt every frame even when nothing moved;
                                  * hjr_render_file only); bit 1: key "verbose" */
    int32_t device_bvh;          /* default 0; 1: key "device_bvh" (the frame data built on the device); 1 + N: that and key
                                  * "device_bvh_refit": N, 0..1000 */
    int32_t device_bvh_opt;      /* default 0; bits 0..7: key "device_bvh_opt", 0..3 treelet-restructuring rounds of that device build;
                                  * bit 8: key "device_bvh_instances"; bit 9: key "device_bvh_graft"; bit 10: key "denoise_variance_spatial";
                                  * bit 11: key "upscale_guided"; bits 12..14: key "denoise_temporal_coverage", 0, 2, 3 or 4; bits 16..22: key
                                  * "firefly_clamp", 0..64; bit 23: key "firefly_clamp_passes"; bit 15: key "denoise_temporal_moments"; bit 24: key "denoise_temporal_response"; bit 25: key "adaptive_temporal"; bit 26: key "morph_targets" (the drivers hand the glTF's morph targets and per-frame weights to the context; default false, as the reference ignores morph data) (bits 10 and up are the section's spare bits:
                                  * those keys have nothing to do with the BVH) */
    uint32_t passes;             /* default 1; 1..64: hjr_render_file / henjou_cli render each frame in this many sample passes, split at
                                  * boundaries rounded down to hjr_sample_granule (empty passes dropped); the PNG is unchanged ("passes") */
    float noise_threshold;       /* default 0 (off); > 0: hjr_render_file / henjou_cli set hjr_adaptive.noise_threshold, render each frame in
                                  * `passes` sample passes (8 when the file has no "passes" key), stop when no tile is active and write the
                                  * PNG from the last pass ("noise_threshold") */
    uint32_t min_samples;        /* default 0 = two granules: hjr_adaptive.min_samples ("min_samples") */
    int32_t denoise_variance;    /* default 0; 1: key "denoise_variance" (the variance-guided filter in Render_mode Denoise /
                                  * DenoiseUpScale2X; ignored in Default); 2: that and key "denoise_temporal" */
} hjr_render_option;
/* hjr_render_option with the render window's keys behind it: the LONGER caller of the sized-struct rule.  hjr_render_option itself keeps its
 * size (callers and tools were built against it); a caller that wants the two keys hands `&w.o` of this struct, with
 * w.o.struct_size = sizeof(hjr_render_option_window) (HJR_INIT_WINDOW), to hjr_load_render_option_window. */
typedef struct hjr_render_option_window {
    hjr_render_option o;
    uint32_t window[4];          /* default 0, 0, 0, 0 (x1 == 0: the whole frame); key "window": [x0, y0, x1, y1], the render window of every frame
                                  * (hjr_params_window.window: full-frame pixels, row 0 at the bottom, x0 and y0 multiples of 8).  hjr_render_file /
                                  * henjou_cli then write PNGs of the window's size: the window's rows and columns of the whole frame's PNG.
                                  * Render_mode Default only */
    uint32_t bucket[2];          /* default 0, 0 (off); key "bucket": [bw, bh], positive multiples of 8: hjr_render_file / henjou_cli render every
                                  * frame (the window, when there is one) bucket by bucket (hjr_bucket_window), compose it on the device
                                  * (hjr_blit_window_device) and download it once; the PNG is unchanged, per-frame chunk-sum memory follows the
                                  * bucket.  Render_mode Default, one process ("devices" 1) */
} hjr_render_option_window;
#define HJR_INIT_WINDOW(s, head) do { memset(&(s), 0, sizeof(s)); (s).head.struct_size = (uint32_t)sizeof(s); } while (0) /* head: o or p */

typedef struct hjr_camera {      /* Params.camera_* (renderer/renderer.h:1187-1191) */
    float pos[3], dir[3], up[3], right[3];
    float f;                     /* camera_f = 2 / tan(fov) (renderer/renderer.h:1147) */
} hjr_camera;

/* Per-launch parameters: the scalar part of `Params` (renderer/renderer.h:1175-1227). */
typedef struct hjr_params {
    uint32_t struct_size;        /* sizeof(hjr_params) of the caller (HJR_INIT) */
    uint32_t width, height;      /* params.image_width/height */
    uint32_t spp;                /* params.spp */
    uint32_t frame;              /* params.frame */
    uint32_t seed;               /* CMJState.scramble (build-defined) */
    uint32_t integrator;         /* HJR_INTEGRATOR_* */
    hjr_camera camera;
    float sky[3];                /* scene_sky_default: the 1x1 IBL texel (renderer/texture.h:58-65) */
    float ibl_intensity;         /* params.ibl_intensity */
    uint32_t rank, world_size;   /* pixel-tile shard: this launch renders the 8x8 tiles whose id t (see hjr_owned_tiles) has t % world_size == rank */
    uint32_t flags;              /* HJR_FLAG_* */
    uint32_t sample_begin, sample_end; /* sample pass of a progressive frame (below); sample_end 0 = the whole frame */
} hjr_params;
/* hjr_params with the render window behind sample_end: the LONGER caller of the sized-struct rule.  hjr_params itself keeps its size; a caller
 * that renders a window hands `&w.p` of this struct, with w.p.struct_size = sizeof(hjr_params_window) (HJR_INIT_WINDOW(w, p)), to any entry
 * point that takes a const hjr_params*.  The library reads the four words behind the hjr_params it knows iff struct_size covers them. */
typedef struct hjr_params_window {
    hjr_params p;
    uint32_t window[4];          /* x0, y0, x1, y1: render window (below); x1 == 0 = the whole frame */
} hjr_params_window;
/* ---- Render window: the pixels of one rectangle of the frame (hjr_params_window.window; DESIGN.md §4 rule 12) ----------------------------
 * window = { x0, y0, x1, y1 }, a half-open rectangle [x0, x1) x [y0, y1) in the kernel's pixel coordinates (row 0 at the bottom, as
 * everywhere).  x1 == 0 (what a plain hjr_params reads as) is the whole frame: that launch is the launch it always was, bit for bit.
 * width and height remain the FULL frame.  A pixel's value depends on its full-frame coordinates, the sample number, the seed and spp only,
 * so a window launch writes the crop of the whole-frame launch, bit for bit, in every AOV.
 * Conditions, else HJR_ERR_ARG with a text that names `window`, and nothing is enqueued or written: x0 < x1 <= width, y0 < y1 <= height, and
 * x0 and y0 multiples of 8 (the window's 8x8 tiles are then tiles of the frame, which the adaptive rule needs); x1 and y1 are free.
 * Every output of a window launch, host or device, is WINDOW-sized: (y1 - y0) x (x1 - x0) elements, row-major, window row 0 first; with
 * HJR_FLAG_PACKED hjr_owned_tiles(x1 - x0, y1 - y0, rank, world_size) x 64 elements on the window's own tile grid.  rank / world_size shard
 * the window's tiles; hjr_get_adaptive_state and hjr_copy_tile_samples speak of the window's tiles.
 * hjr_render[_var] and hjr_render_device[_var] take a window: both kernel families, all integrators, every flag, sample passes, adaptive
 * sampling and both firefly options.  The window is one of the things a continuing sample pass must repeat (else HJR_ERR_STATE).
 * hjr_stats.samples counts window pixels x samples; nan_where stays in full-frame coordinates.  Nothing the context keeps between launches
 * (measured tile costs, adaptive state, running sums, kept chunk sums) is used for another window: pixel bits never depend on what was
 * rendered before.  The filters need neighbours outside the window: hjr_render_denoised, hjr_render_gbuffer*, hjr_denoise_shards_device and
 * any render on a context with option "adaptive_temporal" on refuse a window with HJR_ERR_ARG. */
/* ---- Rendering one frame in sample passes (progressive rendering) ------------------------------------------------
 * sample_end == 0 (what an older, shorter hjr_params reads as), or sample_begin == 0 with sample_end == spp: the whole frame in one launch.
 * Otherwise the call renders samples [sample_begin, sample_end) of the spp-sample frame and writes, to every AOV it is given, the running
 * mean over samples [0, sample_end): running sum * (1.0f / (float)sample_end).  The pass that ends at spp writes the bits of the one-shot
 * frame.  A boundary is a multiple of hjr_sample_granule(spp) or equal to spp, and sample_begin < sample_end <= spp; anything else is
 * HJR_ERR_ARG (a frame of a single chunk, granule == spp, accepts only the whole range).
 * One progressive frame per context:
 *   - a pass with sample_begin == 0 starts it, replacing an unfinished one;
 *   - a pass with sample_begin > 0 continues it: sample_begin must equal the previous pass's sample_end; width, height, spp, frame, seed,
 *     integrator, camera, sky, ibl_intensity, rank, world_size and the flags PACKED, ZERO_UNOWNED and FAST_MATH must be those of the first
 *     pass (STATS may differ from pass to pass), the same set of AOVs must be requested, and the frame data must be unchanged
 *     (hjr_upload_scene, hjr_set_lut, hjr_set_sky, and a hjr_set_transforms / hjr_commit_transforms that replaces the frame data, all end
 *     it; a commit of unchanged transforms does not).  Otherwise the call returns HJR_ERR_STATE, naming the mismatch, enqueues nothing,
 *     writes no output and leaves the frame as it was, so that a corrected call can follow;
 *   - the pass that ends at spp, or any whole-frame render on the context, ends it.
 * Passes are stream-ordered like every launch: the passes of one frame go on one stream (or the caller orders them).  The output pointers
 * may differ from pass to pass; hjr_stats describes the last launch.  hjr_render, hjr_render_device and hjr_render_denoised (which then
 * filters the running mean) all take passes.  Chunk-sum memory is bounded by the pass, plus one running sum per AOV. */
#define HJR_FLAG_STATS 1u        /* run the counting variant of the kernel (slower; fills hjr_stats) */
#define HJR_FLAG_ZERO_UNOWNED 2u /* clear pixels of tiles this rank does not own (for a sum-reduce exchange) */
#define HJR_FLAG_PACKED 4u       /* the AOV buffers (device or host) are PACKED — this rank's tiles only, back to back, each
                                  * tile 64 float4 in row-major 8x8 order (hjr_owned_tiles(..) x 64 float4 per AOV).  What a
                                  * multi-GPU frame exchanges: 1 / world_size of the frame per rank, no zero fill */

#define HJR_FLAG_FAST_MATH 8u    /* opt-in: the approximate-arithmetic kernels — hardware reciprocal / square root / sine / cosine / power and fused
                                  * multiply-adds in the SHADING code, as the reference's own build does (nvcc --use_fast_math: div.approx, sqrt.approx,
                                  * sin.approx in lib/ptx); traversal and ray / triangle test unchanged.  Frames are NOT bit-identical to the default
                                  * (exact) kernels: they agree within the metric's tolerance (per-pixel RMSE < 1e-3 at 1024 spp; tests/test_gpu_fast_math.py).
                                  * Megakernel family only (NEE and Pathtrace); ignored by HJR_FLAG_STATS launches and by MIS launches, whose exact wavefront
                                  * kernels are faster than an approximate megakernel would be (hjr_stats.fast_math tells what ran). */

/* ---- Adaptive sampling: stop converged 8x8 tiles between the sample passes of a frame ---------------------------
 * A setting of the context (like the LUT and the sky), off by default.  It acts on sample passes only: a whole-frame render (sample_end == 0,
 * or [0, spp)) ignores it and is the launch it always was, bit for bit.  With it on, a pass renders only the tiles still ACTIVE; after a pass
 * that ends at n = sample_end with n < spp, n >= min_samples and m = n / hjr_sample_granule(spp) >= 2, every active tile is judged from the
 * spread of its pixels' chunk sums.  Per owned pixel two fp32 statistics over the chunk colour sums c received so far, in chunk order from
 * +0.0f, no contraction:   y = (c.x + c.y) + c.z ;  S1 = S1 + y ;  S2 = S2 + y * y.   Then, all fp32 as written (m, n converted to float):
 *     q = max(m * S2 - S1 * S1, 0.0f) ;   e = sqrt(q / (m - 1.0f)) / (S1 + HJR_ADAPTIVE_EPS * n)
 * (the standard error of the pixel's sum relative to the sum; pixels of an edge tile outside the image have e = 0), the tile's 64 e are
 * added by the xor butterfly v = v + v[lane ^ k], k = 32, 16, 8, 4, 2, 1, and the tile STOPS iff v <= noise_threshold * 64.0f, i.e. its mean
 * relative error is at most the threshold.  A stopped tile never restarts within the frame and keeps n_tile = that sample_end; every pass
 * still writes every owned pixel of every AOV: running sum * (1.0f / (float)n_tile) for a stopped tile, * (1.0f / (float)sample_end)
 * otherwise.  The rule is plain IEEE arithmetic in a fixed order: the result does not depend on rank, GPU count, kernel family or layout.
 * The cancellation in m * S2 - S1 * S1 costs about 1e-7 of S1 * S1, so thresholds below about 1e-3 are accepted but resolve nothing.
 * The next pass needs the number of active tiles to size its launch: an adaptive pass with sample_begin > 0 WAITS on the host for the
 * previous pass of its frame (4 bytes read back).  A pass with no active tile launches no render kernel and still writes the AOVs. */
#define HJR_ADAPTIVE_EPS 1e-3f   /* keeps a black pixel at e = 0 */
typedef struct hjr_adaptive {
    uint32_t struct_size;        /* sizeof(hjr_adaptive) of the caller (HJR_INIT) */
    float noise_threshold;       /* finite, >= 0; 0 = off */
    uint32_t min_samples;        /* no decision before this many samples; 0 = two granules, other values are rounded up to a granule */
} hjr_adaptive;
typedef struct hjr_adaptive_state {
    uint32_t struct_size;        /* sizeof(hjr_adaptive_state) of the caller (HJR_INIT) */
    uint32_t owned_tiles;        /* tiles of this rank */
    uint32_t active_tiles;       /* of them, not stopped after the last pass (the caller stops the frame at 0; the last AOVs are the frame) */
    uint32_t sample_end;         /* where the last pass ended */
    uint64_t samples_rendered;   /* 64 x the sum over the owned tiles of the samples each has received (whole tiles, edge tiles included) */
} hjr_adaptive_state;

/* ---- Variance AOV: a per-pixel error estimate of the colour AOV (hjr_render_var / hjr_render_device_var; DESIGN.md §4 rule 7) ----------
 * An optional fourth output, ONE float per pixel: row-major [height][width]; with HJR_FLAG_PACKED [owned tile][64]; pixels of tiles this
 * rank does not own are untouched, or zeroed with HJR_FLAG_ZERO_UNOWNED, exactly like the colour AOV.  It is computed for every kind of
 * frame (one-shot, sample pass, adaptive) by the streaming kernels after the render; no render kernel knows about it, and the other AOVs
 * of a call with the variance pointer have the bits of the same call without it.  Definition, fp32 in the written order, no contraction,
 * correctly rounded divide:
 *     g = hjr_sample_granule(spp) ;  chunk k is FULL iff (k + 1) * g <= spp ;
 *     per pixel, over the full chunks it has received, in chunk order from +0.0f, with c = the chunk's colour sum as stored:
 *         y = (c.x + c.y) + c.z ;  S1 = S1 + y ;  S2 = S2 + y * y ;      m = the number of those chunks ;
 *     n = the number of samples the written mean is over: spp for a one-shot frame, sample_end on a sample pass, n_tile for a stopped
 *         adaptive tile (whose S1, S2, m are those it stopped with: its variance stays put on later passes) ;
 *     m >= 2:  q = max(m * S2 - S1 * S1, 0.0f) ;  var = (q / (m * (m - 1.0f))) / ((float)g * (float)n)
 *     m <  2:  var = HJR_VARIANCE_UNKNOWN
 * (m, g, n converted to float).  This is the variance of the pixel's mean r + g + b, estimated from the spread of its chunk sums:
 * q / (m (m - 1)) is the sample variance of the chunk sums, / g that of one sample's sum-of-channels scaled to a chunk, / n that of the
 * mean.  The partial last chunk (spp not a multiple of g) is added to the colour as ever and left out of S1 / S2.  m < 2 covers every
 * frame of a single chunk (at most 8 spp: there are no chunk sums at all) and the first one-granule pass of a progressive frame.  A
 * progressive frame keeps S1, S2 per owned pixel between its passes (8 bytes per owned pixel; an adaptive frame uses the statistic it
 * keeps anyway).  "The same set of AOVs on every pass" includes the variance: giving or dropping the pointer on a continuing pass is
 * HJR_ERR_STATE and enqueues nothing. */
#define HJR_VARIANCE_UNKNOWN 1e30f

/* ---- Firefly clamp: a robust per-pixel mean from the chunk sums (option "firefly_clamp" = kappa; DESIGN.md §4 rule 9) -------------------
 * Opt-in and BIASED: it removes energy where rare paths carry it (DESIGN.md gives the measured figures).  Off (0, the default) every call
 * is the call it always was, bit for bit, and launches the same kernels.  With kappa in 1..64 (4 is the recommended value) every
 * WHOLE-FRAME render (hjr_render[_var], hjr_render_device[_var], hjr_render_denoised with sample_end == 0 or [0, spp)) computes the colour
 * AOV as follows, per pixel, fp32 in the written order, no contraction, correctly rounded divide:
 *     g = hjr_sample_granule(spp) ;  m = spp / g (the full chunks) ;  r = spp - m * g (samples of the partial last chunk, if any) ;
 *     c_k = chunk k's colour sum as stored ;  y_k = (c_k.x + c_k.y) + c_k.z ;
 *  1. the rule ACTS iff kappa > 0 and m >= 4; otherwise the frame is the plain frame, bit for bit (every frame of at most 8 spp has no
 *     chunk sums at all, and hjr_sample_granule(spp) = spp there gives m = 1);
 *  2. med = the lower median of y_0 .. y_{m-1}: the value of rank (m - 1) / 2 (integer division) in ascending order; the partial chunk
 *     is not among them;
 *  3. lim = (float)kappa * med + HJR_FIREFLY_EPS * (float)g ;
 *  4. for the partial chunk  lim_r = lim * ((float)r / (float)g) ;
 *  5. in chunk order from +0.0f:  s = (y_k > L) ? L / y_k : 1.0f  with L = lim for a full chunk, lim_r for the partial one;
 *     a.c = a.c + c_k.c * s  for c = x, y, z ;
 *  6. out = a * (1.0f / (float)spp), alpha 1.
 * c * 1.0f is exact, so a pixel none of whose chunks is scaled keeps the plain frame's bits.  Albedo, normal and the variance AOV are
 * untouched: they have the bits of the same call with the option off, and the variance stays the statistic of the RAW chunk sums (it
 * describes the samples, not the clamped mean).  The rule is per pixel and does not depend on rank, GPU count, kernel family or layout:
 * HJR_FLAG_PACKED, HJR_FLAG_ZERO_UNOWNED and sharded launches behave as for the plain frame, and N ranks give the one-rank frame.
 * hjr_stats.firefly_clamped counts the scaled (pixel, chunk) pairs of the launch.
 * The rule needs all chunk sums of a pixel and a progressive frame keeps running sums only: on a context with the option on, a sample
 * pass that is not the whole range [0, spp) is HJR_ERR_ARG (the error names the option); nothing is enqueued or written -- unless option
 * "firefly_clamp_passes" is on:
 *
 * ---- Firefly clamp on sample passes (option "firefly_clamp_passes" = 1 next to "firefly_clamp" = kappa > 0; DESIGN.md §4 rule 10) ---------
 * Off (0, the default), or with "firefly_clamp" 0, every call, refusal, kernel and launch is what the paragraph above says.  With both on
 * a whole-frame render is still that paragraph's, bit for bit, and sample passes are accepted: the context keeps the COLOUR chunk sums of
 * this rank's tiles for the whole progressive frame ([n_chunks][owned tile][64] float4: 16 bytes x n_chunks per owned pixel, where a
 * plain pass keeps those of the pass only; albedo and normal stay per pass with their running sums).  A pass that ends at n = sample_end
 * writes, per owned pixel, with g, c_k, y_k as above, m_n = n / g (integer division: the full chunks received) and r_n = n - m_n * g
 * (non-zero only when n = spp), fp32 in the written order, no contraction, correctly rounded divide and sqrt:
 *  1. the rule ACTS iff m_n >= 4; otherwise the colour has the plain pass's bits;
 *  2. steps 2 - 6 above with m_n, r_n, n in place of m, r, spp: the lower median over y_0 .. y_{m_n-1}, lim = (float)kappa * med +
 *     HJR_FIREFLY_EPS * (float)g, lim_r = lim * ((float)r_n / (float)g), s_k = (y_k > L) ? L / y_k : 1.0f, a.c = a.c + c_k.c * s_k in
 *     chunk order from +0.0f, out = a * (1.0f / (float)n), alpha 1.  The pass that ends at spp therefore writes the one-shot clamped
 *     frame, bit for bit, and a pixel with no scaled chunk keeps the plain pass's bits;
 *  3. albedo, normal and the variance AOV have the bits of the same pass with "firefly_clamp" 0; the variance stays the raw statistic;
 *  4. adaptive frames (hjr_set_adaptive): a pass decides under the conditions stated there, unchanged (n < spp, n >= min_samples,
 *     m_n >= 2).  With m_n < 4 the decision is that rule as it is.  With m_n >= 4 the statistic is that of the CLAMPED sums, recomputed
 *     from the kept chunk sums with this pass's limit:  y'_k = (c_k.x * s_k + c_k.y * s_k) + c_k.z * s_k  (the three products of step 2),
 *     S1' = S1' + y'_k and S2' = S2' + y'_k * y'_k in chunk order from +0.0f over the m_n full chunks; then q, e, the xor butterfly and
 *     v <= noise_threshold * 64.0f as there, with S1', S2'.  A stopped tile holds n_tile: its colour is step 2 over its chunks
 *     [0, n_tile / g) with n = n_tile (the plain mean when those are fewer than 4), the bits it had when it stopped; the chunk slots the
 *     render kernels left stale are never read.  hjr_get_adaptive_state and hjr_copy_tile_samples keep their meaning;
 *  5. hjr_stats.firefly_clamped counts the scaled (pixel, chunk) pairs in the colours the pass wrote, over all in-image owned pixels (a
 *     stopped tile over its own chunks); 0 when the rule did not act;
 *  6. the rule is per pixel and per tile: HJR_FLAG_PACKED, HJR_FLAG_ZERO_UNOWNED, shards, kernel family, layout and integrator do not
 *     enter, and N ranks give the one-rank frame.
 * hjr_render_denoised filters the clamped running mean.  Setting either option (any value) while "firefly_clamp_passes" is on, or that
 * option itself, ends an unfinished progressive frame as hjr_set_adaptive does: a continuing pass after it is HJR_ERR_STATE, with nothing
 * enqueued or written. */
#define HJR_FIREFLY_EPS 1e-3f    /* keeps the limit of a pixel whose median chunk is black above 0 */

typedef struct hjr_stats {
    uint32_t struct_size;        /* sizeof(hjr_stats) of the caller (HJR_INIT) */
    uint32_t _pad0;
    uint64_t samples, closest_rays, shadow_rays, box_tests_closest, tri_tests_closest,
             box_tests_shadow, tri_tests_shadow, shaded_hits, light_samples, nan_samples;
    float    last_kernel_ms;     /* HIP-event time of the last render kernel on its stream */
    uint32_t bvh_nodes, bvh_depth, n_triangles;
    /* which megakernel layout the current frame data selects (csrc/hjr_launch.hip.h::hjr_launch): 0 = BVH4 read from memory,
     * 1 = BVH2 staged in LDS with 32-bit stack entries, 2 = BVH2 in LDS with 16-bit stack entries, 3 = BVH2 read from memory */
    uint32_t lds_mode;
    uint32_t stack_need;         /* worst-case traversal stack entries per lane of the current BVH */
    uint32_t stack_lds_entries;  /* memory-path layouts: entries of a lane's stack kept in LDS; deeper ones overflow to HBM */
    uint32_t pipeline;           /* 0 = persistent megakernel (a lane owns a path), 1 = workgroup-local wavefront kernel (trace / shade batches) */
    uint64_t stack_overflow_pushes; /* HJR_FLAG_STATS launches: stack pushes that went to the HBM overflow (memory-path layouts) */
    /* HJR_FLAG_STATS launches: where NaN / Inf samples came from (they are zeroed and counted in nan_samples; the reference has no
     * guard and would emit a NaN pixel): the first nan_located <= 8 of them in no particular order, as (pixel x, pixel y, sample) */
    uint32_t nan_located;
    uint32_t fast_math;          /* 1: the last launch ran the HJR_FLAG_FAST_MATH kernels */
    uint32_t nan_where[8][3];
    uint32_t bvh_builder;        /* who built the current frame data: 0 = host threads, 1 = device kernels (option "device_bvh") */
    float    frame_build_ms;     /* its build time: host wall time of flatten + BVH build, or HIP-event time of the device build or refit */
    uint32_t bvh_refits;         /* consecutive refits behind the current frame data (option "device_bvh_refit"); 0 = a full build */
    float    bvh_sah;            /* BVH4 SAH of a device-built or refitted tree, computed on the device (Ci 1.2 per inner slot, Ct 1 per triangle
                                  * of a leaf slot, slot area over root area; the same bits every run); 0 for host-built data */
    uint32_t bvh_instances;      /* instance subtrees under the top tree of the current frame data (option "device_bvh_instances");
                                  * 0 = an ordinary build or host-built data */
    float    bvh_topology_ms;    /* HIP-event time of the last per-instance topology build of that option; the commits that reuse the
                                  * topology leave it as it is */
    uint64_t firefly_clamped;    /* option "firefly_clamp": (pixel, chunk) pairs the last whole-frame launch scaled down (with "firefly_clamp_passes": those in the colours the last sample pass wrote); 0 when the rule did not act */
    uint32_t item_chunks;        /* chunks of a pixel per work item of the last render launch (option "item_chunks" as the launch resolved it; 1 for the wavefront kernels) */
    uint32_t _pad1;
    uint32_t morph_vertices;     /* hjr_set_morph: vertices blended for the current frame data by the last commit; 0: no morph, or the blend was skipped
                                  * (the commit reused the frame data, or the working arrays already held these weights over this base) */
    uint32_t _pad2;
    uint64_t geometry_generation; /* the geometry (hjr_update_vertices, hjr_set_morph, hjr_set_morph_weights) the current frame data was built from */
} hjr_stats;

/* ---------------- deforming meshes: per-frame vertex updates and morph targets ----------------
 * A morph set deforms the vertex range [first_vertex, first_vertex + n_vertices) of the uploaded scene with n_targets targets under the
 * weights w[first_weight .. first_weight + n_targets).  Per vertex and per component, in fp32, no contraction, in target order from the base:
 *     p = base;  for k = 0 .. K-1:  p = p + w[k] * d[k]        (the product rounded, then the sum rounded; no target is skipped for a zero weight)
 * Positions take position_deltas, normals normal_deltas (NULL: the set's normals stay at the base).  Normals are not renormalised here: the
 * flatten normalises world normals.  Vertices outside every set keep the base bytes.  The base is what hjr_upload_scene supplied, as last
 * overwritten by hjr_update_vertices.  Sets may share weights (the primitives of one glTF mesh do); sets must not overlap. */
typedef struct hjr_morph_set {
    uint32_t first_vertex, n_vertices, n_targets, first_weight;
    const float* position_deltas; /* float3 x n_targets x n_vertices, target-major: target k of vertex i at 3 * (k * n_vertices + i) */
    const float* normal_deltas;   /* the same shape, or NULL */
} hjr_morph_set;                  /* 32 bytes, fixed layout */
typedef struct hjr_morph {
    uint32_t struct_size;         /* sizeof(hjr_morph) of the caller (HJR_INIT) */
    uint32_t n_sets, n_weights, _pad0;
    const hjr_morph_set* sets;    /* n_sets */
    const float* default_weights; /* n_weights, or NULL: zeros */
} hjr_morph;

typedef struct hjr_scene hjr_scene; /* owning, host side (SceneData + animations) */
typedef struct hjr_ctx hjr_ctx;     /* one per device */

const char* hjr_last_error(void);

/* ---------------- scene surface: the file-level drop-in (host only, no GPU needed) ---------------- */
/* load_json(filepath, RenderOption&) — loader/render_json_loader.h:78-228 (incl. ./fps.txt override, :164-171).
 * `out` must carry its struct_size (HJR_INIT) before the call, like every sized struct. */
int hjr_load_render_option(const char* json_path, hjr_render_option* out);
/* the same with the keys "window" and "bucket" of the "Henjou_HIP" section: `out` is the `o` of a hjr_render_option_window whose struct_size
 * covers the fields it wants (a shorter struct receives what fits, as ever).  hjr_load_render_option checks the two keys and hands out
 * hjr_render_option only: it never writes behind sizeof(hjr_render_option). */
int hjr_load_render_option_window(const char* json_path, hjr_render_option* out);
/* gltfloader(filepath, filename, SceneData&, RenderOption&) — loader/gltfloader.h:1068-1601 */
int hjr_scene_load_gltf(const char* dir, const char* file, hjr_render_option* opt_inout, hjr_scene** out);
void hjr_scene_free(hjr_scene*);
int hjr_scene_get_view(const hjr_scene*, hjr_scene_view* out);
/* Renderer::updateIASMatrix(time) — renderer/renderer.h:257-291: per instance Matrix4x3 + inverse, row-major 3x4 */
int hjr_scene_eval_transforms(const hjr_scene*, float time, float* transforms12, float* inv_transforms12);
/* glTF morph targets ("deforming meshes" above): one set per primitive with `targets` (POSITION and optionally NORMAL, non-sparse FLOAT
 * VEC3; TANGENT is ignored, anything else is a parse error), de-indexed like the vertices; the primitives of a mesh node share the node's
 * weights, whose defaults are mesh.weights.  The pointers are borrowed from the scene.  n_sets == 0: the file has none.  hjr_scene_view is
 * the rest pose either way.  No reference counterpart: the reference ignores morph data. */
int hjr_scene_get_morph(const hjr_scene*, hjr_morph* out);
/* the weights at `time`: the defaults, or the keys of the node's animation channel with "path": "weights", sampled like every other channel
 * (linear, "interpolation" not read, the sampler picked by channel index).  n must equal hjr_morph.n_weights. */
int hjr_scene_eval_morph_weights(const hjr_scene*, float time, float* weights, uint32_t n);
/* camera block of the frame loop — renderer/renderer.h:1145-1169 */
int hjr_scene_eval_camera(const hjr_scene*, const hjr_render_option*, float time, hjr_camera* out);
/* Texture(LUT_path, NonColor) — renderer/texture.h:16-39, loader/texture_load.h:7-20: 8-bit RGBA, caller frees with hjr_free */
int hjr_load_png_rgba8(const char* path, uint8_t** rgba, int* w, int* h);
/* the material-texture form of the same loader: PNG or baseline JPEG by file signature (stbi_load decodes both) */
int hjr_load_image_rgba8(const char* path, uint8_t** rgba, int* w, int* h);
/* HDRTexture(filename, background) — renderer/texture.h:67-100 (stbi_loadf): Radiance .hdr (RGBE) -> float RGBA (a = 0), caller frees with hjr_free */
int hjr_load_hdr_rgba32f(const char* path, float** rgba, int* w, int* h);
void hjr_free(void*);

/* ---------------- device side: replaces context/GAS/IAS/pipeline/SBT + optixLaunch ---------------- */
int hjr_create(int device_ordinal, hjr_ctx** out);                 /* optixDeviceContextInitialize, renderer.h:293-312 */
void hjr_destroy(hjr_ctx*);
/* cpySceneDataToDevice + optixTraversalBuild(GAS) + optixSBTBuild — renderer.h:197-255, 314-396, 620-739 */
int hjr_upload_scene(hjr_ctx*, const hjr_scene_view*);
/* updateIASMatrix + buildIAS — renderer.h:257-291, 398-490.  Flattens to world space and (re)builds the BVH. */
int hjr_set_transforms(hjr_ctx*, const float* transforms12, const float* inv_transforms12, uint32_t n_instances);
/* The same in two halves for pipelined frame loops: hjr_prepare_transforms does the host work (flatten + BVH build, worker
 * threads) into a pending slot and touches neither the device nor anything a running render reads, so it may run on another
 * thread while the previous frame renders; hjr_commit_transforms uploads the pending data and makes it current (call it after
 * that render has finished).  Unchanged transforms (static geometry) are detected and cost nothing. */
int hjr_prepare_transforms(hjr_ctx*, const float* transforms12, const float* inv_transforms12, uint32_t n_instances);
int hjr_commit_transforms(hjr_ctx*);
/* setLUT — renderer.h:854-898 (uchar4, normalised float read, linear, wrap).  NULL clears. */
int hjr_set_lut(hjr_ctx*, const uint8_t* rgba, int w, int h);
/* setSky — renderer.h:802-851: equirect float4 IBL texture (wrap, linear, element read).  NULL restores the 1x1 texel
 * `hjr_params.sky` (scene_sky_default).  Direction -> (u, v): u = atan2(d.z, d.x) / 2pi + 0.5, v = acos(d.y) / pi (build-defined). */
int hjr_set_sky(hjr_ctx*, const float* rgba32f, int w, int h);
/* Deforming meshes (above).  The three calls below take effect at the next hjr_prepare_transforms (hjr_set_transforms), which then is not
 * "unchanged" even with the transforms of the current frame data; they must NOT run concurrently with hjr_prepare_transforms, nor between it
 * and its hjr_commit_transforms.  Like hjr_set_sky they end an unfinished progressive frame (a later pass with sample_begin > 0 is
 * HJR_ERR_STATE), and they drop the temporal history: that stage reprojects rigidly through the instance transforms and cannot follow a
 * deforming surface.  With "device_bvh_instances" they make the next commit build the topology again.  A commit that differs from the
 * previous one only in geometry is a refit under the ordinary policy of "device_bvh_refit".  Errors are HJR_ERR_ARG with hjr_last_error
 * naming the cause, and change nothing.  A vertex made non-finite is caught by the builders ("non-finite vertex after transform"); the
 * previous frame data stays current.  hjr_upload_scene removes the morph.
 * hjr_update_vertices: overwrites [first_vertex, first_vertex + n_vertices) of the base positions, and of the base normals unless `normals`
 * is NULL (float3 each): the entry for deformation the caller computes (skinning, cloth).  The arrays are free on return. */
int hjr_update_vertices(hjr_ctx*, uint32_t first_vertex, uint32_t n_vertices, const float* positions, const float* normals);
/* hjr_set_morph: the morph sets and their default weights; everything is copied.  NULL or n_sets == 0 removes the morph. */
int hjr_set_morph(hjr_ctx*, const hjr_morph*);
/* hjr_set_morph_weights: n must equal hjr_morph.n_weights. */
int hjr_set_morph_weights(hjr_ctx*, const float* weights, uint32_t n);
/* Params fill + optixLaunch + CUDA_SYNC_CHECK + AOV D->H — renderer.h:1175-1242, 103-136.
 * Host buffers, width*height*4 floats each (albedo/normal may be NULL).  Synchronous. */
int hjr_render(hjr_ctx*, const hjr_params*, float* aov_color, float* aov_albedo, float* aov_normal);
/* Same launch writing float4 AOVs straight into caller-owned DEVICE memory (e.g. a torch tensor that then goes
 * through an RCCL collective), enqueued on `hip_stream` (hipStream_t as void*, NULL = default stream).  Asynchronous. */
int hjr_render_device(hjr_ctx*, const hjr_params*, void* d_aov_color, void* d_aov_albedo, void* d_aov_normal,
                      void* hip_stream);
/* hjr_render / hjr_render_device with the variance AOV (above): `aov_variance` is width*height floats (HJR_FLAG_PACKED: owned tiles x 64).
 * A NULL variance pointer makes either call behave exactly like hjr_render / hjr_render_device.  No reference counterpart. */
int hjr_render_var(hjr_ctx*, const hjr_params*, float* aov_color, float* aov_albedo, float* aov_normal, float* aov_variance);
int hjr_render_device_var(hjr_ctx*, const hjr_params*, void* d_aov_color, void* d_aov_albedo, void* d_aov_normal, void* d_aov_variance,
                          void* hip_stream);
int hjr_synchronize(hjr_ctx*);
/* Adaptive sampling of sample passes (above).  NULL or noise_threshold == 0 switches it off (the default).  noise_threshold must be finite
 * and >= 0, else HJR_ERR_ARG.  The call ends an unfinished progressive frame, as hjr_set_sky does, so a frame cannot change its rule half
 * way: a continuing pass after it is refused with HJR_ERR_STATE before anything is enqueued or written.  No reference counterpart (its
 * budget is max_spp under a time limit). */
int hjr_set_adaptive(hjr_ctx*, const hjr_adaptive*);
/* The context's progressive adaptive frame after its last pass so far; synchronous (waits for that pass).  HJR_ERR_STATE when the last
 * render was not an adaptive sample pass. */
int hjr_get_adaptive_state(hjr_ctx*, hjr_adaptive_state* out);
/* n_tile per owned tile of that frame (the samples the tile has received: where it stopped, else where the last pass ended);
 * n_owned_tiles must be hjr_adaptive_state.owned_tiles.  Synchronous. */
int hjr_copy_tile_samples(hjr_ctx*, uint32_t* dst, size_t n_owned_tiles);
/* ---- pixel-tile shard helpers (no reference counterpart: the reference is single-GPU, renderer.h:1077-1078) ----
 * Tiles are 8x8 pixels; tile (tx, ty) has id t = ty * tiles_x + (tx + ty) % tiles_x (row ty of tiles rotated by ty places, so that a
 * rank's tiles run along diagonals instead of forming vertical stripes when tiles_x is a multiple of world_size); tile t belongs to
 * rank t % world_size and is that rank's (t / world_size)-th tile. */
uint32_t hjr_owned_tiles(uint32_t width, uint32_t height, uint32_t rank, uint32_t world_size);
/* Boundary granule of a frame's sample passes (hjr_params.sample_begin / sample_end): the samples of one work-item chunk, 8 up to 512 spp,
 * 16 at 1024, 64 at 4096; spp itself when the frame is a single chunk.  Host only, no GPU needed. */
uint32_t hjr_sample_granule(uint32_t spp);
/* host arrays: row-major float4 frame <-> packed [owned tile][64] float4 of one rank (frame pixels of other ranks untouched) */
int hjr_pack_tiles(const float* frame_rgba, uint32_t width, uint32_t height, uint32_t rank, uint32_t world_size, float* packed_rgba);
int hjr_unpack_tiles(const float* packed_rgba, uint32_t width, uint32_t height, uint32_t rank, uint32_t world_size, float* frame_rgba);
/* the same on device pointers, asynchronous on `hip_stream` (NULL = the context's stream) */
int hjr_pack_tiles_device(hjr_ctx*, const void* d_frame, uint32_t width, uint32_t height, uint32_t rank, uint32_t world_size, void* d_packed, void* hip_stream);
int hjr_unpack_tiles_device(hjr_ctx*, const void* d_packed, uint32_t width, uint32_t height, uint32_t rank, uint32_t world_size, void* d_frame, void* hip_stream);
/* ---- buckets and compositing of render windows (hjr_params_window.window).  Buckets cut a width x height frame into bw x bh rectangles, row-major
 * from (0, 0), the ones at the right and top edge clipped to the frame; bw and bh are positive multiples of 8, so every bucket is a valid
 * window.  hjr_bucket_count: how many (0 for a bad argument).  hjr_bucket_window: bucket `index` as { x0, y0, x1, y1 }; HJR_ERR_ARG for an
 * empty frame, a side that is not a positive multiple of 8, or an index past the end.  Host only, no GPU needed. */
uint32_t hjr_bucket_count(uint32_t width, uint32_t height, uint32_t bw, uint32_t bh);
int hjr_bucket_window(uint32_t width, uint32_t height, uint32_t bw, uint32_t bh, uint32_t index, uint32_t window[4]);
/* window pixels -> frame: the (y1 - y0) x (x1 - x0) float4 image of a window launch is written into rows y0 .. y1 - 1, columns x0 .. x1 - 1 of
 * a width x height float4 frame; the frame's other pixels are untouched.  HJR_ERR_ARG unless x0 < x1 <= width and y0 < y1 <= height (any
 * alignment).  Host form: host pointers, needs no context.  Device form: device pointers, one kernel launch, asynchronous on `hip_stream`
 * (NULL = the context's stream). */
int hjr_blit_window(const float* window_rgba, const uint32_t window[4], float* frame_rgba, uint32_t width, uint32_t height);
int hjr_blit_window_device(hjr_ctx*, const void* d_window, const uint32_t window[4], void* d_frame, uint32_t width, uint32_t height, void* hip_stream);
/* ---- gathered shards -> frames (DESIGN.md §7 "Denoise modes"). What rank 0 holds after the one gather of a frame: world_size blocks, one per
 * rank, rank r's at byte offset r * rank_stride from each of up to four base pointers (rank 0's packed AOVs): colour, albedo and normal as
 * [owned tile][64] float4, the variance AOV as [owned tile][64] float; NULL = absent.  One gather of a per-rank buffer laid out
 * colour | albedo | normal | variance yields exactly this: the pointers are offsets into rank 0's block and rank_stride is the size of the
 * per-rank buffer.  rank_stride is a multiple of 16, and with world_size > 1 at least the size of rank 0's largest block (float4 AOVs:
 * hjr_owned_tiles(w, h, 0, world_size) * 1024 bytes); the float4 pointers are 16-byte aligned.  Only slots of pixels inside the image are
 * read: neither the out-of-image lanes of an edge tile nor the padding behind a rank's last tile.
 * hjr_assemble_shards scatters every block of every AOV into row-major frames (the inverse of the packed layout for all ranks at once);
 * every pixel of every requested output is written exactly once.  An output whose source is NULL must be NULL and the reverse, and at
 * least one AOV must be given, else HJR_ERR_ARG.  Host form: host pointers, needs no context and no GPU.  Device form: device pointers,
 * one kernel launch, asynchronous on `hip_stream` (NULL = the context's stream). */
typedef struct hjr_shards {
    uint32_t struct_size;        /* sizeof(hjr_shards) of the caller (HJR_INIT) */
    uint32_t world_size;         /* N the blocks were rendered with */
    uint64_t rank_stride;        /* bytes from rank r's block to rank r + 1's; the same for all four pointers; a multiple of 16 */
    const void* color;           /* rank 0's packed colour tiles, [owned tile][64] float4; must not be NULL for hjr_denoise_shards_device */
    const void* albedo;          /* NULL = absent */
    const void* normal;
    const void* variance;        /* [owned tile][64] float */
} hjr_shards;
int hjr_assemble_shards(const hjr_shards*, uint32_t width, uint32_t height, float* color, float* albedo, float* normal, float* variance);
int hjr_assemble_shards_device(hjr_ctx*, const hjr_shards*, uint32_t width, uint32_t height, void* d_color, void* d_albedo, void* d_normal,
                               void* d_variance, void* hip_stream);
/* OptixDenoiserManager::layerSet + denoise() — renderer/denoiser.h:42-189, renderer/renderer.h:1093-1120, 1258-1270:
 * (aov_color | guide albedo | guide normal) of in_w x in_h -> AOV_Output of out_w x out_h.  The OptiX AI network is closed, so
 * this is a REPLACEMENT with the same data flow, not a reproduction of its pixels: HJR_MODE_DEFAULT copies
 * (blendFactor 1), HJR_MODE_DENOISE runs a 5-pass edge-avoiding a-trous filter guided by the two AOVs (out size == in size),
 * HJR_MODE_DENOISE_UPSCALE2X filters at (out_w / 2, out_h / 2) (renderer.h:1096-1099) and upscales 2x bilinearly. */
int hjr_denoise(hjr_ctx*, int render_mode, uint32_t in_w, uint32_t in_h, const float* aov_color, const float* aov_albedo,
                const float* aov_normal, float* out, uint32_t out_w, uint32_t out_h);
/* One frame of the loop in any render mode, kept on the device: launch at p->width x p->height (the caller halves it for
 * DenoiseUpScale2X, renderer.h:1096-1099), hjr_denoise_device (option "denoise_variance" 1: the variance AOV too and
 * hjr_denoise_var_device), download of AOV_Output only (renderer.h:1229-1281).  Synchronous. */
int hjr_render_denoised(hjr_ctx*, const hjr_params*, int render_mode, float* out, uint32_t out_w, uint32_t out_h);
/* The same frame from the gathered shards of a multi-GPU render instead of from a render (rank 0 of henjou_cli's multi-GPU path):
 * hjr_assemble_shards_device into the context's AOV buffers, then exactly what hjr_render_denoised runs after its render, under the same
 * context options: with "denoise_temporal" the G-buffer pass (of the context's current frame data: rank 0 has set the frame's transforms),
 * the accumulation against the context's history and its commit (a whole frame, or the pass that ends at spp); then the filter, plain or
 * variance-guided, and in DenoiseUpScale2X the upscale.  The output has the bits of hjr_render_denoised: shards only move data.
 * `frame` describes the WHOLE frame: width x height (the render size), camera, spp, sample_begin / sample_end (which pass of the frame the
 * shards hold; 0 / 0 = the whole frame); its rank, world_size and HJR_FLAG_PACKED are ignored, gathered->world_size says how the blocks were
 * made.  Device pointers; every stage is asynchronous on `hip_stream` (NULL = the context's stream); d_out is out_w x out_h float4.
 * HJR_ERR_ARG: HJR_MODE_DEFAULT (nothing to filter: hjr_assemble_shards_device is the whole job) or an unknown mode, a missing colour, albedo
 * or normal block, a variance block the options need ("denoise_variance" / "denoise_temporal") and the shards lack, bad sizes or sample range.
 * HJR_ERR_STATE: "denoise_temporal" without current frame data.  In every error case nothing is enqueued.  No reference counterpart. */
int hjr_denoise_shards_device(hjr_ctx*, const hjr_params* frame, int render_mode, const hjr_shards* gathered, void* d_out, uint32_t out_w,
                              uint32_t out_h, void* hip_stream);
/* the same on device pointers (float4 images), asynchronous on `hip_stream` (NULL = the context's stream) */
int hjr_denoise_device(hjr_ctx*, int render_mode, uint32_t in_w, uint32_t in_h, const void* d_color, const void* d_albedo,
                       const void* d_normal, void* d_out, uint32_t out_w, uint32_t out_h, void* hip_stream);
/* The variance-guided variant of the filter (the spatial half of SVGF, Schied et al. 2017; csrc/hjr_denoise.hip.h has the arithmetic to
 * the bit): `aov_variance` is in_w*in_h floats, the variance AOV of hjr_render_var (or any per-pixel variance of the colour's r + g + b;
 * NaN and negative values act as 0, HJR_VARIANCE_UNKNOWN as "no estimate": guides only).  The colour tolerance of a pixel is 4 standard
 * deviations, so the filter fades out as the frame converges, where hjr_denoise keeps its bias.  Same modes, size rules and argument
 * checks as hjr_denoise / hjr_denoise_device; the variance is required in the two Denoise modes; HJR_MODE_DEFAULT copies. */
int hjr_denoise_var(hjr_ctx*, int render_mode, uint32_t in_w, uint32_t in_h, const float* aov_color, const float* aov_albedo,
                    const float* aov_normal, const float* aov_variance, float* out, uint32_t out_w, uint32_t out_h);
int hjr_denoise_var_device(hjr_ctx*, int render_mode, uint32_t in_w, uint32_t in_h, const void* d_color, const void* d_albedo,
                           const void* d_normal, const void* d_variance, void* d_out, uint32_t out_w, uint32_t out_h, void* hip_stream);
/* The spatial variance estimate (what SVGF does while its history is short; csrc/hjr_denoise.hip.h has the arithmetic to the bit, DESIGN.md
 * §11.3 what was measured): the variance AOV needs two full chunks of a pixel, so a frame of at most 8 spp, and a first one-granule sample
 * pass, carry HJR_VARIANCE_UNKNOWN everywhere.  Every pixel whose input variance is unknown (>= HJR_VARIANCE_UNKNOWN after the filter's
 * clamp, +Inf included) gets the guide-weighted variance of the luminance r + g + b over its 3 x 3 neighbourhood (the filter's normal and
 * albedo weights, indices clamped to the frame); every other pixel keeps its input bits, NaN and negative values too.  An estimate that is
 * not below HJR_VARIANCE_UNKNOWN is written as HJR_VARIANCE_UNKNOWN.  variance_in NULL = every pixel unknown.  w x h float4 colour, albedo and
 * normal, w x h float variances.  HJR_ERR_ARG before anything is enqueued: a null colour, guide or output, an empty image, a side above
 * 16384.  hjr_estimate_variance: host pointers, synchronous.  hjr_estimate_variance_device: device pointers, one launch, asynchronous on
 * `hip_stream` (NULL = the context's stream); d_variance_out may be d_variance_in (in place: a pixel's input is read by the lane that writes
 * it only). */
int hjr_estimate_variance(hjr_ctx*, uint32_t w, uint32_t h, const float* aov_color, const float* aov_albedo, const float* aov_normal,
                          const float* variance_in, float* variance_out);
int hjr_estimate_variance_device(hjr_ctx*, uint32_t w, uint32_t h, const void* d_color, const void* d_albedo, const void* d_normal,
                                 const void* d_variance_in, void* d_variance_out, void* hip_stream);
/* ---- Temporal accumulation with reprojection (the temporal half of SVGF; csrc/hjr_temporal.hip.h has the arithmetic to the bit, DESIGN.md
 * §11.2 the rule, its limits and what was measured).  Two stateless building blocks and a context option that chains them.
 * G-buffer: the first hit of every pixel's centre ray (no RNG; the ray of the tile classifier) against the context's current frame data,
 * either builder, every layout option.  One 48-byte record per pixel, row-major; a miss is prim = 0xffffffff and zeros elsewhere.  `pos` is the
 * hit point as the closest-hit program computes it, `ng` the world-space geometric normal cross(v1 - v0, v2 - v0), not normalised.
 * hjr_render_gbuffer reads width, height and camera of hjr_params only.  HJR_ERR_STATE without frame data; HJR_ERR_ARG for world_size > 1,
 * HJR_FLAG_PACKED or an empty image.  Host form synchronous; device form asynchronous on `hip_stream` (NULL = the context's stream). */
typedef struct hjr_gbuffer_px { uint32_t prim, inst; float t, b1, b2; float pos[3]; float ng[3]; uint32_t pad; } hjr_gbuffer_px; /* 48 bytes */
int hjr_render_gbuffer(hjr_ctx*, const hjr_params*, hjr_gbuffer_px* out);
int hjr_render_gbuffer_device(hjr_ctx*, const hjr_params*, void* d_out, void* hip_stream);
/* The coverage G-buffer: the same records, bit for bit, except `pad`.  After the centre ray every pixel traces side x side
 * sub-pixel rays on a regular grid (no RNG; `side` is 2, 3 or 4) and counts those that land on the centre ray's surface: both miss, or both
 * hit the same instance and the same material within one pixel footprint of the centre's tangent plane.  pad = same | (side * side) << 8;
 * a miss record carries its counts too.  A pixel with same < side * side straddles two surfaces ("mixed").  Refuses what hjr_render_gbuffer
 * refuses, and a `side` outside {2, 3, 4} with HJR_ERR_ARG, before anything is enqueued. */
int hjr_render_gbuffer_cov(hjr_ctx*, const hjr_params*, uint32_t side, hjr_gbuffer_px* out);
int hjr_render_gbuffer_cov_device(hjr_ctx*, const hjr_params*, uint32_t side, void* d_out, void* hip_stream);
/* Accumulation: per pixel of the current frame, the surface point is taken back to object space with the current inverse transform of its
 * instance, forward with the previous transform, and projected with the previous camera; four bilinear taps of the previous frame's
 * accumulated colour, variance and history length are kept if they show the same instance and the same surface point (plane distance and
 * in-plane distance against the pixel footprint), and the current colour is blended in with alpha = max(1 / h, HJR_TEMPORAL_ALPHA),
 * h = min(h_prev + 1, 64).  The variance is propagated as that of a convex combination of independent estimates; HJR_VARIANCE_UNKNOWN or NaN
 * on either side gives HJR_VARIANCE_UNKNOWN, negative values act as 0.  A miss, a disocclusion or prev == NULL restarts the pixel:
 * out = cur colour, cur variance, h = 1.  A sized struct describes either side; all pointers of one call are host pointers
 * (hjr_temporal_accumulate, synchronous) or device pointers (hjr_temporal_accumulate_device, asynchronous on `hip_stream`).  cur.history is
 * ignored.  width, height and n_instances must agree between the two sides, else HJR_ERR_ARG.  Outputs: float4 colour (alpha = cur's),
 * float variance, float history length, width x height each.  Caller-made records are range-checked before any table lookup: an instance
 * or prim id out of range is a miss (current pixel) or an invalid tap; prim ids are checked against the uploaded scene's triangle count.
 * Coverage (`coverage` != 0 on a side: its records' `pad` words are hjr_render_gbuffer_cov's; 0, or a caller whose struct ends before the
 * field: the pad words are ignored and the rule is the one above, bit for bit).  A record of a side with coverage is mixed iff
 * total = (pad >> 8) & 0xff is above 0 and (pad & 0xff) < total.  A current pixel that is not mixed takes no tap whose previous record is
 * mixed.  A current pixel that is mixed keeps its history only from the previous pixel it coincides with: the reprojected position must lie
 * within HJR_TEMPORAL_SNAP of a pixel centre in x and in y, that pixel is the only tap (weight 1, the usual validity tests) and, if the
 * previous side carries coverage, its pad word must equal the current one; otherwise the pixel restarts.  pad is only compared, never an
 * index.
 * Temporal moments (hjr_temporal_accumulate_moments[_device] with out_moments != NULL): SVGF's temporal variance estimate.
 * Every pixel also carries the accumulated first and second moment (m1, m2: float2, width x height) of the luminance l = (r + g) + b of the
 * current frame's colour.  A restarting pixel starts them at (l, l * l); otherwise the taps that carry the colour carry the previous
 * moments with the same weights, and l and l * l are blended in with the colour's alpha.  Once the pixel's history length h has reached
 * HJR_TEMPORAL_MOMENTS_MIN the output variance is not the propagated one but
 *   max(m2 - m1 * m1, 0) * k / (1 - k),  k = max(1 / h, HJR_TEMPORAL_ALPHA / (2 - HJR_TEMPORAL_ALPHA)):
 * the unbiased weighted sample variance of one frame's luminance, scaled by the sum of the squared blend weights to the variance of the
 * accumulated colour (approximate where bilinear mixing made h fractional).  A difference that is not finite, or a product that is not
 * below HJR_VARIANCE_UNKNOWN, is HJR_VARIANCE_UNKNOWN.  Below the threshold the variance is the propagated one, "unknown" included.  The
 * coverage rules choose the taps as without moments.  Moments are only multiplied, added and compared: NaN, Inf or huge caller-made values
 * cannot fault.  The previous frame's moments are the argument prev_moments (hjr_temporal_frame itself is unchanged: its size and its last
 * field, `coverage`, are part of the ABI callers were built against); out_moments == NULL is hjr_temporal_accumulate[_device], bit for bit
 * and the same launch, and prev_moments is then ignored; out_moments != NULL with a prev != NULL and prev_moments == NULL is HJR_ERR_ARG
 * and nothing is enqueued; with prev == NULL prev_moments is ignored.
 * Response to moving light (hjr_temporal_accumulate_response[_device] with out_response != NULL).  Reprojection follows
 * geometry and cameras, not illumination: a shadow or a light that moves over a surface lags in the history by about 1 / alpha frames.  A
 * pixel that keeps its history ("carried") compares, over the (2 R + 1)^2 window around it, the mean of the current luminance with the mean
 * of the reprojected history's luminance, over the window's carried pixels of its own instance, and judges the difference against the
 * standard error of the current frame's window mean:  t = |mean(cur - history)| / (sqrt(var(cur) / n) + EPS),
 * lambda = clamp((t - T0) / (T1 - T0), 0, 1), 0 with fewer than NMIN such pixels.  The blend factor becomes max(alpha, lambda) for colour,
 * variance and moments, and where lambda > 0 the history length falls to at most 1 / that factor: at lambda = 1 the pixel takes the current
 * frame and starts over.  out_response receives lambda (float, width x height; 0 in pixels that restart).  out_response == NULL is
 * hjr_temporal_accumulate_moments[_device], bit for bit and the same launch; with out_moments == NULL as well it is
 * hjr_temporal_accumulate[_device].  The rules for prev_moments are those above.  Where lambda = 0 in a pixel its outputs are the bits of
 * the call without out_response.  Luminances are only added, multiplied, divided and compared: hostile values give lambda in [0, 1]. */
#define HJR_TEMPORAL_ALPHA 0.2f  /* the published value */
#define HJR_TEMPORAL_SNAP 0.125f /* a mixed pixel's reprojection may lie this many pixels off a pixel centre, per axis */
#define HJR_TEMPORAL_MOMENTS_MIN 4.0f /* history length from which the variance comes from the moments (the published switch) */
#define HJR_TEMPORAL_RESP_R 2       /* the response window is (2 R + 1)^2 pixels */
#define HJR_TEMPORAL_RESP_T0 3.0f   /* standard errors of the window mean below which a change is one frame's noise: lambda = 0 */
#define HJR_TEMPORAL_RESP_T1 6.0f   /* ... and from which the history is dropped: lambda = 1 */
#define HJR_TEMPORAL_RESP_NMIN 5    /* fewer window members than this: lambda = 0 */
#define HJR_TEMPORAL_RESP_EPS 1e-3f /* added to the standard error: a noiseless window answers only to a change above T0 * EPS */
typedef struct hjr_temporal_frame {
    uint32_t struct_size, width, height, n_instances;
    hjr_camera camera;
    const float *transforms12, *inv_transforms12;   /* n_instances x 12, as hjr_set_transforms */
    const hjr_gbuffer_px* gbuffer;
    const float *color /* float4 */, *variance /* float */, *history /* float: frames accumulated */;
    uint32_t coverage;                              /* != 0: the G-buffer's pad words are coverage counts (hjr_render_gbuffer_cov) */
} hjr_temporal_frame;
int hjr_temporal_accumulate(hjr_ctx*, const hjr_temporal_frame* prev /* NULL = none */, const hjr_temporal_frame* cur, float* out_color,
                            float* out_variance, float* out_history);
int hjr_temporal_accumulate_device(hjr_ctx*, const hjr_temporal_frame* prev, const hjr_temporal_frame* cur, void* d_out_color, void* d_out_variance,
                                   void* d_out_history, void* hip_stream);
int hjr_temporal_accumulate_moments(hjr_ctx*, const hjr_temporal_frame* prev /* NULL = none */, const hjr_temporal_frame* cur, float* out_color,
                                    float* out_variance, float* out_history, const float* prev_moments /* float2, of prev */,
                                    float* out_moments /* float2; NULL = hjr_temporal_accumulate */);
int hjr_temporal_accumulate_moments_device(hjr_ctx*, const hjr_temporal_frame* prev, const hjr_temporal_frame* cur, void* d_out_color,
                                           void* d_out_variance, void* d_out_history, const void* d_prev_moments, void* d_out_moments,
                                           void* hip_stream);
int hjr_temporal_accumulate_response(hjr_ctx*, const hjr_temporal_frame* prev /* NULL = none */, const hjr_temporal_frame* cur, float* out_color,
                                     float* out_variance, float* out_history, const float* prev_moments /* float2, of prev */,
                                     float* out_moments /* float2; NULL = without moments */,
                                     float* out_response /* float; NULL = hjr_temporal_accumulate_moments */);
int hjr_temporal_accumulate_response_device(hjr_ctx*, const hjr_temporal_frame* prev, const hjr_temporal_frame* cur, void* d_out_color,
                                            void* d_out_variance, void* d_out_history, const void* d_prev_moments, void* d_out_moments,
                                            void* d_out_response, void* hip_stream);
/* The prior (csrc/hjr_temporal.hip.h section PRIOR; adaptive sampling's rule 11 below reads it): what the history will contribute to each
 * pixel of a frame that has not been rendered yet.  out_prior is float4 (lp, vp, al, 0), width x height.  The reprojection, the taps and
 * their validity tests (and the coverage rules when a side's `coverage` is set) are hjr_temporal_accumulate's, bit for bit, up to the
 * gathered c_prev, v_prev, h_prev.  A pixel that keeps its history, with no tap of unknown variance, gets
 *   h = min(max(h_prev + 1, 1), 64),  al = max(1 / h, HJR_TEMPORAL_ALPHA),  lp = (c_prev.r + c_prev.g) + c_prev.b,  vp = v_prev;
 * every other pixel (a restart, prev == NULL, an unknown variance in a tap) gets (0, 0, 1, 0).  al is the factor the accumulation will blend
 * the pixel's colour with.  The response's lambda and the temporal moments do not enter: they need the current frame's colour.  The
 * arguments and their checks are hjr_temporal_accumulate's, except that cur->color and cur->variance are not read and may be NULL (cur
 * needs its G-buffer, camera and transforms).  hjr_temporal_prior: host pointers, synchronous; hjr_temporal_prior_device: device pointers,
 * asynchronous on `hip_stream`. */
int hjr_temporal_prior(hjr_ctx*, const hjr_temporal_frame* prev /* NULL = none */, const hjr_temporal_frame* cur, float* out_prior /* float4 */);
int hjr_temporal_prior_device(hjr_ctx*, const hjr_temporal_frame* prev, const hjr_temporal_frame* cur, void* d_out_prior, void* hip_stream);
/* The guided 2x upscale (csrc/hjr_denoise.hip.h has the arithmetic to the bit, DESIGN.md §11.4 what was measured): a joint-bilateral stand-in
 * for the bilinear upscale of HJR_MODE_DENOISE_UPSCALE2X.  Every pixel of the out_w x out_h output takes the four bilinear taps (weights 0.75 /
 * 0.25, clamped indices) of the in_w x in_h colour image and keeps those whose low-resolution G-buffer record shows the surface of the output
 * pixel's own record: both misses, or the same instance, the tap's point within one low-resolution pixel footprint of the output pixel's
 * tangent plane, and normals within acos(0.9).  The kept taps are renormalised; a pixel whose four taps all pass, or all fail, has the bits
 * of the bilinear upscale.  gbuffer_lo (in_w x in_h) and gbuffer_hi (out_w x out_h) come from hjr_render_gbuffer with the one camera `cam`;
 * records are compared, never used as indices, so caller-made ones cannot fault.  out_w / 2 == in_w and out_h / 2 == in_h (integer
 * division; odd output sizes are legal).  HJR_ERR_ARG before anything is enqueued: a null pointer, an empty image, sizes that break the
 * rule, an output side above 8192 (the G-buffer's limit).  hjr_upscale_guided: host pointers, synchronous.  hjr_upscale_guided_device: device
 * pointers (cam stays a host pointer, read during the call), one launch, asynchronous on `hip_stream` (NULL = the context's stream). */
int hjr_upscale_guided(hjr_ctx*, uint32_t in_w, uint32_t in_h, const float* color_lo, const hjr_gbuffer_px* gbuffer_lo, const hjr_camera* cam,
                       const hjr_gbuffer_px* gbuffer_hi, float* out, uint32_t out_w, uint32_t out_h);
int hjr_upscale_guided_device(hjr_ctx*, uint32_t in_w, uint32_t in_h, const void* d_color_lo, const void* d_gbuffer_lo, const hjr_camera* cam,
                              const void* d_gbuffer_hi, void* d_out, uint32_t out_w, uint32_t out_h, void* hip_stream);
/* Drops the history that option "denoise_temporal" keeps in the context: the next frame restarts everywhere.  So do hjr_upload_scene,
 * hjr_set_lut, hjr_set_sky, a change of width, height or render mode, and setting the option. */
int hjr_temporal_reset(hjr_ctx*);
/* The 8-bit preview buffer of the raygen program — `uchar4* image` of Params, allocated at renderer/renderer.h:1102 and bound at :1175, written
 * by the missing __raygen__rg and never read back by the host.  Build-defined: a float4 colour image on the device -> tonemapper of kernel/color.h
 * (HJR_TONEMAP_*) -> toSRGB + quantise (renderer.h:73-101) -> width*height RGBA8 on the device; asynchronous on `hip_stream` (NULL = the
 * context's stream).  The host form is hjr_tonemap_to_srgb8; device pow / exp may differ from libm by one code value at a quantisation boundary. */
int hjr_preview_device(hjr_ctx*, const void* d_color, uint32_t width, uint32_t height, int tonemap, void* d_rgba8, void* hip_stream);
int hjr_get_stats(hjr_ctx*, hjr_stats* out);
/* Tuning / test options of a context.  The library reads NO environment variable: kernel selection and layouts depend on the scene, the
 * launch parameters and these options only.  value -1 = the library's default; HJR_ERR_ARG for an unknown key or a value out of range.
 *   key               values      meaning (default)
 *   "pipeline"        0 1 2       kernel family: 0 per launch what was measured faster (wavefront kernels for MIS, megakernel otherwise; default),
 *                                 1 persistent megakernel, 2 workgroup-local wavefront kernel
 *   "lds_bvh"         0 1         1: stage BVH2 + triangles in LDS when they fit (default), 0: always read the scene from memory     [*]
 *   "lds_stack16"     0 1         1: 16-bit LDS traversal-stack entries whenever the tree admits them (default: only when 32-bit ones do not fit) [*]
 *   "bvh_width"       2 4         force the node format; 4 also forces the memory path (default: BVH2 in LDS when it fits, BVH4 otherwise)   [*]
 *   "leaf_max"        1..4        triangles per BVH leaf (2)                                                                        [*]
 *   "bvh_refine"      0..16       insertion-based refinement passes over the built BVH2, largest subtrees first (0 up to 65536 triangles, 1 above) [*]
 *   "node_min"        1..64       traversal descent loops: lanes still descending below which a pass moves on to the leaves (6 / 8 / 24 by layout and family)
 *   "hold_min"        0..64       megakernel, LDS layouts: metallic hits a wave collects before it shades them; 0 never holds (8)
 *   "hold_age"        1..1000     ... or rounds the oldest of them has waited (2)
 *   "short_stack"     1..64       memory layouts: traversal-stack entries per lane kept in LDS, deeper ones overflow to HBM (16)
 *   "blocks_per_cu"   1..8        memory layouts: workgroups per CU of the persistent grid (occupancy query)
 *   "top_nodes"       0..1024     memory layouts, BVH4: nodes of the top of the tree every workgroup also keeps in LDS (85 = levels 0 - 3; 0 none)
 *   "tile_order"      0 1 2       0 plain tile order, 1 first-hit classes, 2 classes + measured cost of the previous frame (1 on one GPU, 2 when sharded)
 *   "wf_cap"          64..32768   wavefront kernel: path contexts per workgroup, a power of two (2048 in LDS layouts, 4096 otherwise)
 *   "wf_refill" / "wf_prefetch_min" / "wf_trace_min"   wavefront kernel: hand-over thresholds of the trace stage, scheduler preference
 *   "host_threads"    1..256      worker threads of the per-frame host preparation, process-wide (min(hardware threads, 16))
 *   "verbose"         0 1         BVH format, sizes, host build stages per frame, one line per sample pass on stderr (0)
 *   "force_rebuild"   0 1         rebuild the frame data even when the transforms did not change (0)
 *   "device_bvh"      0 1         0: flatten + BVH build on host threads (default); 1: on the device, as kernels on the context's stream
 *                                 (Morton-order tree collapsed to BVH4, always the memory layout: lds_mode 0).  hjr_prepare_transforms then
 *                                 only validates and builds the light table; hjr_commit_transforms runs the build and makes its result
 *                                 current only if it succeeds.  Rejected together with a forced "bvh_width" 2 or "lds_bvh" 1;
 *                                 "bvh_refine" does not apply                                                                  [*]
 *   "device_bvh_opt"  0..3        with "device_bvh" 1: treelet-restructuring rounds over the device-built BVH2 before the collapse
 *                                 (Karras & Aila 2013; 0 = the plain Morton tree, the default).  Same frames, a better tree: on a 1 M-triangle
 *                                 scene 1 round took the build from 5.5 to 10.4 ms and the render from 151 to 135 ms.  The host build
 *                                 ignores it                                                                                   [*]
 *   "device_bvh_refit" 0..1000    with "device_bvh" 1: after a full device build, up to this many consecutive commits keep its topology and
 *                                 refit it (new triangles in the same leaf order, node boxes bottom-up, one host wait) instead of building;
 *                                 the next commit builds again.  Frames do not depend on the tree, so they stay the same bits.  A commit
 *                                 refits only while the current data is a device build or refit of the same uploaded scene under the same
 *                                 build options and instance count, the scene has at least 2 triangles and the cost guard below holds;
 *                                 "force_rebuild" still only means "do not skip unchanged transforms".  hjr_stats.bvh_refits / bvh_sah
 *                                 report it; bvh_builder stays 1.  0 (default): every commit builds.  The host build ignores it        [*]
 *   "device_bvh_refit_growth" 0..10000  percent (default 10): when a refit's tree cost (hjr_stats.bvh_sah) exceeds the last full build's by
 *                                 more than this, the NEXT commit is a full build; the refit just made stays current                   [*]
 *   "device_bvh_instances" 0 1    with "device_bvh" 1: the topology of every instance's triangles is built once per uploaded scene and build
 *                                 options (object space, "device_bvh_opt" rounds inside an instance) and kept on the device; every commit
 *                                 flattens in that leaf order, recomputes the boxes inside the instance subtrees, builds a top tree over the
 *                                 instances' world boxes (at most 1024 non-empty instances) and collapses to one world-space BVH4.  Same
 *                                 frames; rigid motion never degrades the tree.  "device_bvh_refit" / "device_bvh_refit_growth" are ignored
 *                                 with it (hjr_stats.bvh_refits stays 0); hjr_stats.bvh_instances / bvh_topology_ms report it.  More than
 *                                 1024 non-empty instances, or a top tree deeper than the traversal stack, silently take the ordinary build
 *                                 (bvh_instances 0).  0 (default): the ordinary build.  The host build ignores it                    [*]
 *   "device_bvh_graft" 0 1        with "device_bvh" 1 and "device_bvh_instances" 1: the BVH4 of every instance of more than "leaf_max"
 *                                 triangles is collapsed once with the topology, from the object-space boxes, and kept instead of the
 *                                 binary tree; every commit flattens, recomputes those nodes' boxes bottom-up, builds a BVH4 top tree over
 *                                 the instances' world boxes and puts the instances' nodes behind it.  Same frames; the nodes differ from
 *                                 those of "device_bvh_instances" alone.  The same fallbacks and the same hjr_stats fields
 *                                 (bvh_topology_ms includes the one-off collapse).  Accepted and without effect when either of the two
 *                                 other options is off.  0 (default)                                                                [*]
 *   "denoise_variance" 0 1        1: hjr_render_denoised renders the variance AOV along with the guides and runs the variance-guided filter
 *                                 (hjr_denoise_var_device) in the two Denoise modes; a sample pass filters the running mean with the variance
 *                                 over n = sample_end.  0 (default): today's call, bit for bit
 *   "denoise_temporal" 0 1        1: hjr_render_denoised in the two Denoise modes renders guides and the variance AOV (whatever "denoise_variance"
                                 says), runs the G-buffer pass, accumulates against the history the context keeps (hjr_temporal_accumulate's
                                 rule), and hands the accumulated colour and variance to the variance-guided filter; DenoiseUpScale2X keeps the
                                 history at the render size.  A whole-frame render, or the sample pass that ends at spp, makes the current
                                 frame the previous one; an earlier sample pass reads the history and does not advance it.  The caller
                                 advances hjr_params.frame between frames: the same frame number twice blends identical samples and the
                                 propagated variance then understates.  world_size > 1 or HJR_FLAG_PACKED is HJR_ERR_ARG with it (a sharded
                                 frame goes through hjr_denoise_shards_device, which honours both options); HJR_MODE_DEFAULT ignores it.  Setting it (any value) drops the history.  0 (default): today's call, bit for bit
   "firefly_clamp"  0..64        kappa of the firefly clamp (above, "Firefly clamp"): whole-frame renders scale every chunk sum of a pixel that
                                 exceeds kappa x the lower median of the pixel's full chunks down to that limit.  Biased, opt-in; 4 is the
                                 recommended value.  Sample passes other than [0, spp) are HJR_ERR_ARG with it unless "firefly_clamp_passes"
                                 is on.  0 (default): today's call, bit for bit, the same kernels
   "firefly_clamp_passes" 0 1    1: with "firefly_clamp" > 0 sample passes and adaptive frames are accepted (above, "Firefly clamp on sample
                                 passes"): the context keeps the colour chunk sums of the whole progressive frame (16 bytes x chunks of the
                                 frame per owned pixel: 1.06 GB at 1080p x 256 spp on one GPU), every pass of at least 4 full chunks writes
                                 the clamped running mean, and an adaptive frame stops on the statistic of the clamped sums.  Whole-frame
                                 renders are unchanged.  Without effect while "firefly_clamp" is 0.  Setting it (any value), or
                                 "firefly_clamp" while it is 1, ends an unfinished progressive frame.  0 (default): today's calls and
                                 refusals, bit for bit, the same launches
   "item_chunks"    1 2 4 8      megakernel: consecutive sample chunks of one pixel that form a work item of the queue.  A launch uses the
                                 largest power of two that is no larger than this and divides the number of chunks it renders (possibly 1).
                                 Scheduling only: every chunk is still summed on its own, frames are the same bits.  Default: 1 for launches
                                 with world_size > 1 (short, tail-bound) and for counting launches (HJR_FLAG_STATS), else what was measured
                                 fastest on one GPU (csrc/hjr_render.hip: HJR_ITEM_CHUNKS).  The wavefront kernels and MIS always run single chunks;
                                 hjr_stats.item_chunks reports what the last launch used
   "denoise_variance_spatial" 0 1  1: with "denoise_variance" or "denoise_temporal" on, hjr_render_denoised and hjr_denoise_shards_device run
                                 hjr_estimate_variance_device in place on the frame's variance AOV before the temporal stage and the filter:
                                 pixels of unknown variance (every pixel of a frame of at most 8 spp or of a first one-granule sample pass) get
                                 the 3 x 3 estimate, and the temporal stage propagates it by its own rule; a known variance is untouched, so
                                 from 16 spp on the frame is the same bits as with 0.  Accepted and without effect when neither of the two
                                 other options is on, and in HJR_MODE_DEFAULT.  The variance AOV of hjr_render_var is not changed by it.
                                 Setting it (any value) drops the temporal history.  0 (default): today's call, bit for bit, the same launches
   "upscale_guided" 0 1          1: hjr_render_denoised and hjr_denoise_shards_device in HJR_MODE_DENOISE_UPSCALE2X run the filter as today with its
                                 last pass into a buffer at the render size, trace the G-buffer at the render size (the one "denoise_temporal"
                                 traced for this frame is reused) and at out_w x out_h from the same hjr_params.camera, and run
                                 hjr_upscale_guided_device instead of the bilinear upscale, all on the call's stream.  Composes with the filter
                                 options, sample passes, adaptive passes and "firefly_clamp"; the temporal history stays at the render size.
                                 hjr_render_denoised with world_size > 1 or HJR_FLAG_PACKED is HJR_ERR_ARG with it, hjr_denoise_shards_device
                                 without current frame data HJR_ERR_STATE, an output side above 8192 HJR_ERR_ARG, each before anything is
                                 enqueued.  The other modes ignore it; the stateless hjr_denoise[_var][_device] have no camera and keep the
                                 bilinear upscale.  0 (default): today's call, bit for bit, the same launches
   "denoise_temporal_coverage" 0 2 3 4  with "denoise_temporal" on: 2, 3 or 4 make hjr_render_denoised and hjr_denoise_shards_device run the
                                 coverage pass (hjr_render_gbuffer_cov_device with that side) in place of the plain G-buffer pass, keep the coverage
                                 records in the history slots and accumulate with `coverage` set on both sides (rules 2' and 3' of
                                 csrc/hjr_temporal.hip.h).  1 and values above 4 are HJR_ERR_ARG.  No effect unless "denoise_temporal" is on.
                                 Setting it (any value) drops the temporal history.  0 (default): today's call, bit for bit, the same launches
   "denoise_temporal_moments" 0 1  1: with "denoise_temporal" on, hjr_render_denoised and hjr_denoise_shards_device keep a moments buffer in each of
                                 the two history slots and accumulate with hjr_temporal_accumulate_moments_device: from a history length of
                                 HJR_TEMPORAL_MOMENTS_MIN on a pixel's variance comes from its own luminance history.  Meant for frames of at
                                 most 8 spp together with "denoise_variance_spatial", which supplies the variance of shorter histories (without
                                 it those stay "unknown").  A sample pass that does not end the frame computes the moments and discards them.
                                 No effect unless "denoise_temporal" is on.  Setting it (any value) drops the temporal history.  0 (default):
                                 today's call, bit for bit, the same launches
   "denoise_temporal_response" 0 1  1: with "denoise_temporal" on, hjr_render_denoised and hjr_denoise_shards_device accumulate with
                                 hjr_temporal_accumulate_response_device: where the window mean of the current luminance leaves that of the
                                 reprojected history by more than HJR_TEMPORAL_RESP_T0 standard errors of one frame, the history gives way
                                 (illumination that moves over a surface no longer lags).  Composes with "denoise_temporal_coverage",
                                 "denoise_temporal_moments", "denoise_variance_spatial", sample passes and "firefly_clamp".  No effect unless
                                 "denoise_temporal" is on.  Setting it (any value) drops the temporal history.  0 (default): today's call, bit
                                 for bit, the same launches
   "adaptive_temporal" 0 1       1: adaptive sampling counts the temporal history (rule 11).  In effect only on a sample pass of an
                                 adaptive frame (hjr_set_adaptive, threshold > 0) rendered by hjr_render_denoised in a Denoise mode with
                                 "denoise_temporal" on; every other call is today's, bit for bit and the same launches.  At the frame's first
                                 pass the G-buffer is traced and hjr_temporal_prior_device gathers (lp, vp, al) per pixel from the history; a
                                 frame without history has no prior and is rule 6's frame, bit for bit.  With a prior, on a deciding pass
                                 (rule 6's conditions) hjr_finalize_kernel decides nothing and hjr_adaptive_temporal_kernel decides behind it,
                                 per pixel of an active tile, fp32 as written, n = sample_end, g the granule, m = n / g, (S1, S2) the raw statistic:
                                   e6 = rule 6's e;   if al < 1:   lc = S1 / n,   vc = rule 7's variance of the mean (S1, S2, m, g, n),
                                   om = 1 - al,   va = (om om) vp + (al al) vc,   la = lp + (lc - lp) al,
                                   ea = sqrt(va) / (max(la, 0) + HJR_ADAPTIVE_EPS),   e = min(ea, e6)  (a NaN ea gives e6);   else e = e6;
                                 the tile sum is rule 6's butterfly and the tile stops iff sum <= noise_threshold x 64.  e <= e6, so a tile
                                 never receives more samples than under rule 6 on the same frame, history and passes.  The prior leaves
                                 out "denoise_temporal_response"'s lambda and "denoise_temporal_moments"; the accumulation still applies
                                 them.  A pass that leaves no active tile commits the temporal history as the pass that ends at spp does;
                                 a pass that continues such a frame is HJR_ERR_STATE with nothing enqueued (the next pass starts a new frame).
                                 Together with "firefly_clamp" > 0 and "firefly_clamp_passes" 1 the call is HJR_ERR_ARG before anything is
                                 enqueued (rules 10 and 11 would both decide).  Setting it ends an unfinished progressive frame, as
                                 hjr_set_adaptive does, and keeps the history.  hjr_denoise_shards_device ignores it
   [*] takes effect at the next hjr_set_transforms / hjr_prepare_transforms.
 * Not a context option: "passes" (1..64, default 1) is a key of the file's "Henjou_HIP" section (hjr_render_option.passes): hjr_render_file
 * and henjou_cli render each frame in that many sample passes (hjr_params.sample_begin / sample_end) and write the same PNG.  Nor are
 * "noise_threshold" / "min_samples" of the same section (hjr_render_option.noise_threshold / min_samples -> hjr_set_adaptive).
 * Seventeen more keys of that section set the context option of their name; where each is stored is in the comment on hjr_render_option.
 * "force_rebuild" is set by hjr_render_file only.  "verbose", "device_bvh", "device_bvh_refit": N (integer 0..1000), "device_bvh_opt",
 * "device_bvh_instances", "device_bvh_graft", "firefly_clamp": N (integer 0..64) and "firefly_clamp_passes" (true, false, 0 or 1; a parse
 * error without "firefly_clamp") are set single-GPU and on every rank of --devices N.
 * "denoise_variance", "denoise_temporal" (both in the two Denoise modes only), "denoise_variance_spatial", "upscale_guided",
 * "denoise_temporal_moments", "denoise_temporal_response", "adaptive_temporal" (all three true, false, 0 or 1; "adaptive_temporal" is a parse error without "denoise_temporal": true, and henjou_cli --devices N > 1 refuses it: the ranks decide per shard without a history) and "denoise_temporal_coverage": N (0, 2, 3 or 4) are set single-GPU and on rank 0 of --devices N, which filters, accumulates and upscales (the
 * PNG is the single-GPU run's).  "device_bvh_refit" and "device_bvh_instances" are a parse error without "device_bvh": true, and
 * "device_bvh_graft" without "device_bvh_instances": true; "device_bvh_instances", "device_bvh_graft" and "upscale_guided" take true, false, 0
 * or 1 only.  "denoise_variance_spatial", "denoise_temporal_coverage", "denoise_temporal_moments" and "denoise_temporal_response" are accepted and without effect without "denoise_variance" /
 * "denoise_temporal", "upscale_guided" outside DenoiseUpScale2X.  Both drivers refuse, before they load the scene or touch a device:
 * "denoise_temporal" together with "noise_threshold" > 0 unless "adaptive_temporal" is true (an adaptive frame that stops early never
 * reaches the pass that advances the history; with the key the pass that stops the last tile commits it), and "firefly_clamp" together with "passes" > 1 or "noise_threshold" > 0 unless "firefly_clamp_passes" is true (the rule needs
 * every chunk sum of a pixel and a frame in sample passes keeps running sums only).  An option call that fails ends the job.
 * No reference counterpart (OptiX owns these decisions); tests use them to force every kernel layout. */
int hjr_set_option(hjr_ctx*, const char* key, int value);
int hjr_get_option(hjr_ctx*, const char* key, int* value);
/* Synchronous copy of the current frame data (either builder) for inspection: `what` is one of HJR_FRAME_*; dst NULL asks for the size
 * only (*bytes), otherwise dst_bytes must hold it.  Layouts: csrc/hjr_layout.h.  No reference counterpart (OptiX keeps its GAS opaque). */
enum { HJR_FRAME_NODES = 0, HJR_FRAME_TRI_GEOM = 1, HJR_FRAME_TRI_SHADE = 2, HJR_FRAME_LIGHTS = 3 };
int hjr_copy_frame_data(hjr_ctx*, int what, void* dst, size_t dst_bytes, size_t* bytes);
/* Host-only self-test of the 16-bit traversal-stack encoding (csrc/hjr_traverse.hip.h): 0 when every child ref of a tree the
 * builder admits to that layout survives encode + decode.  No reference counterpart (OptiX owns its traversal stack). */
int hjr_selftest_stack16(void);
/* Ray-batch test hook: hands caller-chosen rays to the software traversal of the render kernels, against the frame data the context
 * currently holds, and returns what it found (tests/test_gpu_trace.py compares that with a brute force over all triangles, bit for bit).
 * Pair i is a shadow (any-hit) ray and a closest-hit ray; either may be invalid (valid == 0).  tmax is read for the shadow ray only: the
 * closest-hit ray ends at 1e16 and both start at tmin = 0.001, as in the render loop.  Rays are traced as given: no normalisation.
 * out[i] holds the shadow ray's `occluded` and the closest-hit ray's hit: global prim id, its row k in the leaf-ordered triangle array
 * (HJR_FRAME_TRI_GEOM), t and the barycentrics; prim == 0xffffffff and zeros mean no hit.
 * The launch uses the megakernel layout a render would get under the context's options ("lds_bvh", "lds_stack16", "bvh_width", "short_stack",
 * "top_nodes", "node_min", "leaf_max", "device_bvh", "device_bvh_opt" all apply), builds the same per-lane stacks and runs the same LDS
 * staging; the kernels (csrc/hjr_trace_hook.hip.h) call the traversal functions unchanged.  `path` selects the loop:
 *   HJR_TRACE_STANDALONE  the stand-alone traversal (MIS' BSDF-sampled ray, the tile classifier): any-hit for the shadow ray, then closest hit;
 *   HJR_TRACE_FUSED       the fused two-ray traversal with the layout's straggler carry-over and the launch's node_min, driven in rounds like
 *                         the render loop by a small persistent grid (one workgroup for the LDS layouts, two for the memory layouts): a lane
 *                         takes the next pair when its previous one is resolved, a lane still in flight resumes next to the others' fresh pairs;
 *   HJR_TRACE_WAVEFRONT   NOT BUILT: returns HJR_ERR_ARG.  The wavefront kernel's trace stage takes its rays from parked path contexts
 *                         whose two rays share one origin (or the launch's camera position) and whose hit record has no t, so it cannot be
 *                         handed independent rays, nor return t, without changing the stage's own code; the frame-level comparison of the
 *                         two kernel families (tests/test_gpu_variants.py) stays its check.
 * `path | HJR_TRACE_FAST_BUILD` runs the instantiation of the same kernels that is compiled with the flags of the HJR_FLAG_FAST_MATH render
 * kernels; its results must equal the exact build's, bit for bit.
 * status: HJR_TRACE_STATUS_OK; HJR_TRACE_STATUS_ROUND_CAP when a wave of the fused path gave up after 2 n + 64 rounds with the pair still in
 * flight (every round resolves at least one lane, so this is never expected); HJR_TRACE_STATUS_UNTRACED for a pair no lane took after that.
 * Checks, in this order and all before any launch: the path (HJR_ERR_ARG: unknown, or HJR_TRACE_WAVEFRONT), null ray / result pointers with
 * n > 0 (HJR_ERR_ARG), n > 2^24 (HJR_ERR_ARG), a null context (HJR_ERR_ARG), no frame data (HJR_ERR_STATE — also for n == 0), a
 * HJR_TRACE_FAST_BUILD the build does not have (HJR_ERR_ARG).  A call that passes them with n == 0 does nothing and returns HJR_OK.
 * Synchronous.  The call overwrites part of the context's hjr_stats: stack_overflow_pushes, lds_mode, stack_need and stack_lds_entries then
 * describe THIS launch.  If a render's counters are still pending (an asynchronous hjr_render_device not yet followed by hjr_get_stats) they
 * are fetched first, so that they do not land on top of the hook's values later; those four fields of that render are then lost — read a
 * render's statistics before tracing.  No reference counterpart. */
typedef struct hjr_ray { float o[3]; float tmax; float d[3]; uint32_t valid; } hjr_ray;                                    /* 32 bytes */
typedef struct hjr_ray_result { uint32_t occluded, prim, k; float t, b1, b2; uint32_t status, pad; } hjr_ray_result; /* 32 bytes */
enum { HJR_TRACE_STANDALONE = 0, HJR_TRACE_FUSED = 1, HJR_TRACE_WAVEFRONT = 2, HJR_TRACE_FAST_BUILD = 0x100 };
enum { HJR_TRACE_STATUS_OK = 0, HJR_TRACE_STATUS_ROUND_CAP = 1, HJR_TRACE_STATUS_UNTRACED = 2 };
int hjr_trace_rays(hjr_ctx*, int path, uint32_t n, const hjr_ray* shadow, const hjr_ray* closest, hjr_ray_result* out);

/* ---------------- output stage (host) ---------------- */
/* float4ConvertColor: toSRGB + quantizeUnsignedChar — renderer/renderer.h:73-101 */
int hjr_float4_to_srgb8(const float* rgba, uint8_t* out_rgba8, uint32_t n_pixels);
/* Preview-buffer tonemappers of kernel/color.h: HJR_TONEMAP_UCHIMURA (color.h:10-53), HJR_TONEMAP_ACES (color.h:55-63),
 * applied per channel before the sRGB + quantise stage above (the raygen code that used them is missing: build-defined order). */
enum { HJR_TONEMAP_NONE = 0, HJR_TONEMAP_UCHIMURA = 1, HJR_TONEMAP_ACES = 2 };
int hjr_tonemap_to_srgb8(const float* rgba, uint8_t* out_rgba8, uint32_t n_pixels, int tonemap);
/* sutil::saveImage(name, buffer, false) — renderer.h:1291-1302.  flip_y != 0 writes row 0 at the bottom. */
int hjr_write_png(const char* path, const uint8_t* rgba8, uint32_t width, uint32_t height, int flip_y);
int hjr_write_pfm(const char* path, const float* rgba, uint32_t width, uint32_t height);
/* Renderer::initializeAndRender(render_option_path) — renderer/renderer.h:1053-1317, whole file-to-PNG path */
int hjr_render_file(const char* render_option_json, int device_ordinal);

#ifdef __cplusplus
}
#endif
#endif
