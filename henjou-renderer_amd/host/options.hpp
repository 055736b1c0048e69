// Tuning / test options of a device context (include/henjou_hip.h: hjr_set_option / hjr_get_option).  The default build of the library reads
// NO environment variable: behaviour depends on its arguments only.  Experiment builds (`make variant`, -DHJR_ENV_OPTIONS) additionally
// take every option from the environment at hjr_create (HJR_<KEY IN UPPER CASE>), so that one binary can be swept from a shell script.
#pragma once
#include <cstdint>
#include <cstring>

namespace hjr {

enum Opt {
    OPT_PIPELINE, OPT_LDS_BVH, OPT_LDS_STACK16, OPT_BVH_WIDTH, OPT_LEAF_MAX, OPT_NODE_MIN, OPT_HOLD_MIN, OPT_HOLD_AGE, OPT_SHORT_STACK,
    OPT_BLOCKS_PER_CU, OPT_TILE_ORDER, OPT_WF_CAP, OPT_WF_REFILL, OPT_WF_PREFETCH_MIN, OPT_WF_TRACE_MIN, OPT_HOST_THREADS, OPT_VERBOSE,
    OPT_FORCE_REBUILD, OPT_TOP_NODES, OPT_BVH_REFINE, OPT_DEVICE_BVH, OPT_DEVICE_BVH_OPT, OPT_DENOISE_VARIANCE, OPT_DENOISE_TEMPORAL, OPT_DEVICE_BVH_REFIT,
    OPT_DEVICE_BVH_REFIT_GROWTH, OPT_DEVICE_BVH_INSTANCES, OPT_DEVICE_BVH_GRAFT, OPT_FIREFLY_CLAMP, OPT_ITEM_CHUNKS, OPT_DENOISE_VARIANCE_SPATIAL,
    OPT_UPSCALE_GUIDED, OPT_DENOISE_TEMPORAL_COVERAGE, OPT_FIREFLY_CLAMP_PASSES, OPT_DENOISE_TEMPORAL_MOMENTS,
    OPT_DENOISE_TEMPORAL_RESPONSE, OPT_ADAPTIVE_TEMPORAL,
    OPT_COUNT
};
struct OptDesc { const char* key; int lo, hi; };
// value -1 always means "the library's default"; the ranges are those of explicit values
inline const OptDesc* opt_table()
{
    static const OptDesc t[OPT_COUNT] = {
        { "pipeline", 0, 2 },        // 0 per launch what was measured faster (wavefront kernels for MIS, megakernel otherwise), 1 megakernel, 2 wavefront kernel
        { "lds_bvh", 0, 1 },         // 1 stage BVH2 + triangles in LDS when they fit (default), 0 always read the scene from memory       [next hjr_set_transforms]
        { "lds_stack16", 0, 1 },     // 1 prefer 16-bit LDS stack entries whenever the tree admits them (default: only when 32-bit ones do not fit) [next hjr_set_transforms]
        { "bvh_width", 2, 4 },       // 2 / 4: force the node format (4 also forces the memory path); 3 is rejected                       [next hjr_set_transforms]
        { "leaf_max", 1, 4 },        // triangles per BVH leaf (default 2)                                                              [next hjr_set_transforms]
        { "node_min", 1, 64 },       // descent loops: lanes still descending below which a pass moves on to the leaves (default 6 / 8 / 24 by layout and kernel family)
        { "hold_min", 0, 64 },       // megakernel, LDS layouts: metallic hits a wave collects before it shades them (0 never holds; default 8)
        { "hold_age", 1, 1000 },     // ... or rounds the oldest of them has waited (default 2)
        { "short_stack", 1, 64 },    // memory layouts: traversal-stack entries per lane kept in LDS (default 16; deeper ones overflow to HBM)
        { "blocks_per_cu", 1, 8 },   // memory layouts: workgroups per CU of the persistent grid (default: what the occupancy query returns)
        { "tile_order", 0, 2 },      // 0 plain tile order, 1 first-hit classes, 2 classes + measured cost of the previous frame (default 1 at N = 1, 2 at N > 1)
        { "wf_cap", 64, 32768 },     // wavefront kernel: path contexts per workgroup, a power of two (default 2048 / 4096)
        { "wf_refill", 1, 64 },      // wavefront kernel: hand-over threshold of the trace stage, lanes without a ray
        { "wf_prefetch_min", 1, 64 },// ... lanes that have used up their prefetched context
        { "wf_trace_min", 1, 4096 }, // wavefront kernel: queued rays from which the scheduler prefers TRACE
        { "host_threads", 1, 256 },  // worker threads of the per-frame host preparation (default min(hardware threads, 16)); process-wide
        { "verbose", 0, 1 },         // 1: BVH format, sizes and host build time per frame on stderr
        { "force_rebuild", 0, 1 },   // 1: rebuild the frame data even when the transforms did not change (benchmarking)
        { "top_nodes", 0, 1024 },    // memory layouts, BVH4: nodes of the top of the tree every workgroup also stages in LDS (0 none)
        { "bvh_refine", 0, 16 },     // insertion-based refinement passes over the built BVH2 (default 0 up to 65536 triangles, 1 above)  [next hjr_set_transforms]
        { "device_bvh", 0, 1 },      // 0 host build (default), 1 flatten + BVH4 build on the device (memory layout; bvh_refine ignored)  [next hjr_set_transforms]
        { "device_bvh_opt", 0, 3 },  // device_bvh 1: treelet-restructuring rounds over the device-built BVH2 (default 0; host build ignores it) [next hjr_set_transforms]
        { "denoise_variance", 0, 1 },// 1: hjr_render_denoised renders the variance AOV and runs the variance-guided filter (default 0: the plain filter)
        { "denoise_temporal", 0, 1 },// 1: hjr_render_denoised accumulates over frames with reprojection in front of the variance-guided filter (default 0)
        { "device_bvh_refit", 0, 1000 },         // device_bvh 1: consecutive commits after a full device build that refit its tree instead of building (default 0; host build ignores it) [next hjr_set_transforms]
        { "device_bvh_refit_growth", 0, 10000 }, // ... percent by which a refit's tree cost may exceed the last full build's before the next commit builds again (default 10) [next hjr_set_transforms]
        { "device_bvh_instances", 0, 1 },        // device_bvh 1: per-instance trees built once per scene, a top tree over them per commit (default 0; host build ignores it; refits are off with it) [next hjr_set_transforms]
        { "device_bvh_graft", 0, 1 },            // device_bvh 1 and device_bvh_instances 1: every instance's BVH4 collapsed once and grafted under a BVH4 top tree per commit (default 0; ignored otherwise) [next hjr_set_transforms]
        { "firefly_clamp", 0, 64 },              // kappa of the firefly clamp on whole-frame renders: chunk sums above kappa x the pixel's median chunk are scaled down to it (default 0 = off; 4 recommended; biased)
        { "item_chunks", 1, 8 },                 // megakernel: consecutive chunks of a pixel in one work item: 1, 2, 4 or 8; a launch uses the largest power of two <= this that divides its chunk count (default: measured per launch kind, hjr_render.hip: launch_render)
        { "denoise_variance_spatial", 0, 1 },    // "denoise_variance" / "denoise_temporal" on: 1 fills pixels whose variance is unknown (frames of at most 8 spp, a first one-granule pass) with a 3 x 3 guide-weighted estimate in front of the temporal stage and the filter (default 0; no effect otherwise)
        { "upscale_guided", 0, 1 },              // 1: DenoiseUpScale2X of hjr_render_denoised / hjr_denoise_shards_device traces G-buffers at the render and the output size and runs the guided upscale (hjr_upscale_guided) instead of the bilinear one (default 0; the other modes ignore it)
        { "denoise_temporal_coverage", 0, 4 },   // "denoise_temporal" on: 2, 3 or 4 run the coverage G-buffer pass with that many sub-pixel rays per side and the coverage-aware accumulation rules (default 0; 1 is rejected; no effect otherwise)
        { "firefly_clamp_passes", 0, 1 },        // "firefly_clamp" on: 1 accepts sample passes and adaptive frames, keeps the colour chunk sums of the whole progressive frame and clamps every pass of >= 4 full chunks; an adaptive frame stops on the clamped statistic (default 0: passes refused; no effect with "firefly_clamp" 0)
        { "denoise_temporal_moments", 0, 1 },    // "denoise_temporal" on: 1 keeps the luminance moments (m1, m2) per pixel in the history and takes the variance from them once a pixel's history length reaches HJR_TEMPORAL_MOMENTS_MIN (default 0; no effect otherwise)
        { "denoise_temporal_response", 0, 1 },   // "denoise_temporal" on: 1 accumulates with the windowed change test (hjr_temporal_accumulate_response_device): where the current frame's window mean of the luminance leaves the reprojected history's, the history gives way (default 0; no effect otherwise)
        { "adaptive_temporal", 0, 1 },           // "denoise_temporal" on and hjr_set_adaptive: 1 lets the sample passes of hjr_render_denoised stop a tile on the error of the ACCUMULATED pixel (DESIGN.md §4 rule 11) and commits the history when the last tile stops (default 0; no effect otherwise; refused with an acting "firefly_clamp_passes")
    };
    return t;
}
// values inside an option's range that it refuses all the same
inline bool opt_hole(int i, int value)
{
    return (i == OPT_BVH_WIDTH && value == 3) || (i == OPT_DENOISE_TEMPORAL_COVERAGE && value == 1) || ((i == OPT_WF_CAP || i == OPT_ITEM_CHUNKS) && (value & (value - 1)) != 0);
}
inline int opt_find(const char* key)
{
    if (!key) return -1;
    const OptDesc* t = opt_table();
    for (int i = 0; i < OPT_COUNT; i++) if (strcmp(t[i].key, key) == 0) return i;
    return -1;
}
struct Options {
    int v[OPT_COUNT];
    Options() { for (int& x : v) x = -1; }
    int get(Opt o, int def) const { return v[o] < 0 ? def : v[o]; }
    bool is_set(Opt o) const { return v[o] >= 0; }
};
// what host/frame.cpp needs of them
struct BuildOptions {
    bool allow_lds = true, prefer_stack16 = false, timing = false;
    int bvh_width = -1, leaf_max = -1, refine = -1;
};
void set_host_threads(int n); // host/frame.cpp; n <= 0 restores the default

} // namespace hjr
