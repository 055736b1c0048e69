// Device context of the C-ABI (hjr_ctx) and the records the device-layer units hand each other: work area layout, build key, sized parameters, the plan of a
// render launch.  Plain declarations: no kernel is declared or included here (hjr_launch.hip.h turns a LaunchPlan into a kernel of its translation unit).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/henjou_hip.h"
#include "../host/frame.hpp"
#include "../host/options.hpp"
#include "hjr_bvh_build.h"
#include "hjr_params.hip.h"

namespace hjr {
void set_error(const std::string& s);
}
using hjr::set_error;

// Work area (d_work, zeroed before every launch), byte offsets.  The diagnostic builds (HJR_TIMING, HJR_WF_WATCHDOG) write their slots
// as P.stats[HJR_NSTAT + i], so those follow the counters directly.
struct WorkArea {
    static constexpr size_t QUEUE_HEAD = 0;                      // uint32 work-queue head (16 bytes)
    static constexpr size_t STATS = 16;                          // HJR_NSTAT uint64 counters (hjr_stats)
    static constexpr size_t DIAG = STATS + HJR_NSTAT * 8;        // 26 uint64: phase clocks / lane-occupancy sums / draw-site counts / watchdog record
    static constexpr size_t TILE_COUNT = DIAG + 26 * 8;          // 8 uint32 tile-class counters (hjr_aux.hip.h)
    static constexpr size_t COST_HIST = TILE_COUNT + 32;         // 128 uint32: cost histogram and bucket cursors (hjr_aux.hip.h)
    static constexpr size_t NAN_LIST = COST_HIST + 512;          // uint64 count, then HJR_NAN_LIST located samples
    static constexpr size_t FIREFLY = NAN_LIST + (1 + HJR_NAN_LIST) * 8; // uint64: (pixel, chunk) pairs scaled by hjr_firefly_kernel (hjr_aux.hip.h)
    static constexpr size_t BYTES = FIREFLY + 8;
};

// The build options frame data depends on, as hjr_prepare_transforms read them: frame data is reused for unchanged transforms, refitted, or
// its instance topology kept, only under an equal key.
struct BuildKey {
    bool allow_lds = true, prefer_stack16 = false;  // options "lds_bvh", "lds_stack16"
    int bvh_width = -1, leaf_max = -1, refine = -1; // "bvh_width", "leaf_max", "bvh_refine" as set (-1: the builder's default)
    bool device = false;                            // "device_bvh": hjr_commit_transforms runs the build; without it the three below stay 0
    uint32_t opt_rounds = 0;                        // "device_bvh_opt"
    bool instances = false, graft = false;          // "device_bvh_instances", and under it "device_bvh_graft"
    // One word per key, one-to-one over the options' ranges: what Refit::tag and the builder's topology cache compare.  Composed here only;
    // nothing takes it apart.
    uint32_t pack() const
    {
        return (uint32_t)allow_lds | ((uint32_t)prefer_stack16 << 1) | ((uint32_t)(bvh_width + 1) << 2) | ((uint32_t)(leaf_max + 1) << 6) | ((uint32_t)(refine + 1) << 10) |
               ((uint32_t)device << 16) | (opt_rounds << 17) | ((uint32_t)instances << 19) | ((uint32_t)graft << 20);
    }
    bool operator==(const BuildKey& o) const { return pack() == o.pack(); }
};

// hjr_params as the library keeps it: the caller's hjr_params with the render window behind it, the layout of hjr_params_window
// (include/henjou_hip.h); take_params (hjr_device_internal.h) fills it from either caller
struct ParamsW : hjr_params { uint32_t window[4]; };
static_assert(sizeof(ParamsW) == sizeof(hjr_params_window) && sizeof(hjr_params) % 4 == 0, "ParamsW must have the layout of hjr_params_window");

struct hjr_ctx {
    int device = 0;
    int n_cus = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hjr::SceneCopy scene;
    bool have_scene = false, have_frame = false;
    // what the frame data currently on the device was built from
    struct Built {
        std::vector<float> m, inv; // instance transforms
        BuildKey key;
    } built;
    // what hjr_prepare_transforms hands to hjr_commit_transforms, which makes it current
    struct Prepared {
        bool valid = false;   // a prepare succeeded and no commit has taken it yet
        bool same = false;    // transforms and key equal `built`: the commit keeps the frame data, nothing below was written
        hjr::FrameData frame; // host build: the frame data.  key.device: the counts and the host-built light table; the commit runs the build
        std::vector<float> m, inv;
        BuildKey key;
        double build_ms = 0.0; // host wall time of the prepare (a device build: replaced by its HIP-event time)
    } prep;
    hjr::FrameData frame; // device-built frame data: the counts, format and lights only (the arrays live in d_nodes, d_tri_*)
    hjr::DeviceBvh dbvh;  // the device builder's scene copy, scratch and pending output buffers
    // option "device_bvh_refit": what the next commit needs to know about the current frame data
    struct Refit {
        bool device = false;   // it came from a device build or refit (of the scene dbvh holds while dbvh.have_scene)
        bool rebuild = false;  // the growth guard tripped: the next commit is a full build
        uint32_t tag = 0;      // build tag of its last full build
        uint32_t count = 0;    // consecutive refits behind it
        float sah = 0.0f, sah_full = 0.0f; // its tree cost, its last full build's
    } refit;
    DevBuf d_nodes, d_tri_geom, d_tri_shade, d_tri_inst, d_materials, d_lights, d_lut, d_work;
    DevBuf d_texels, d_tex_desc, d_srgb_lut, d_sky;
    int sky_w = 0, sky_h = 0;
    uint32_t n_textures = 0;
    int lut_w = 0, lut_h = 0;
    DevBuf d_color, d_albedo, d_normal; // staging for hjr_render (host buffers)
    DevBuf d_bucket[2]; // hjr_render_file, "bucket": the frame being composed | the bucket being rendered
    DevBuf d_part_color, d_part_albedo, d_part_normal; // chunk sums [pass_chunks][owned tile][64] float4 (colour under rule 10: [n_chunks], kept across the passes of a frame)
    DevBuf d_run_color, d_run_albedo, d_run_normal; // running sums of a frame rendered in sample passes, [owned tile][64] float4
    DevBuf d_stat; // per owned pixel (S1, S2) of such a frame, [owned tile][64] float2; allocated at the first adaptive pass or pass with a variance
    DevBuf d_spill; // overflow of the short traversal stacks (memory-path kernels)
    DevBuf d_wf_ctx; // context planes of the wavefront kernel
    DevBuf d_tiles; // [tile_order | tile_class] of the cost-ordered tile list
    DevBuf d_tile_cost; // measured per-tile cost of the previous frame
    uint64_t cost_tag = 0; // (width, height, spp, rank, world, integrator) the costs belong to; 0 = none
    uint64_t cost_rect = 0; // ... and the work rectangle (WorkRect::key; 0 = the whole frame)
    uint32_t cost_samples = 0; // samples per pixel of the launch that measured them (a whole frame or a sample pass)
    DevBuf d_dn_a, d_dn_b, d_dn_out; // denoise ping-pong / host-entry staging
    // variance AOV (hjr_render_var) and variance-guided filter (hjr_denoise_var); nothing here is allocated before a call asks for a variance
    DevBuf d_variance;         // staging for the host-buffer entry points, one float per pixel
    DevBuf d_dnv_a, d_dnv_b;   // the filter's variance ping-pong, one float per pixel
    DevBuf d_ug_lo, d_ug_hi;   // option "upscale_guided": the G-buffers at the render size (unless the temporal stage traced it) and at the output size
    hjr_stats stats;
    bool event_pending = false;
    // Frame data generation: hjr_upload_scene, hjr_set_lut, hjr_set_sky and a commit that replaces the frame data bump it, so a frame
    // rendered in sample passes can tell that what it renders changed between two passes
    uint64_t frame_gen = 0;
    // The one frame of this context that is being rendered in sample passes (hjr_params.sample_begin / sample_end):
    // the parameters of its first pass, the sample its next pass must start at, the AOVs it writes (bit 0 colour, 1 albedo, 2 normal, 3 variance)
    // and the frame data generation it was started on
    struct PassSession {
        bool active = false;
        ParamsW p;
        uint32_t next = 0, aovs = 0;
        uint64_t gen = 0;
        bool committed = false; // option "adaptive_temporal": the frame ended when its last tile stopped and its history was committed (cleared by the next pass that is enqueued)
    } pass;
    // Adaptive sampling (hjr_set_adaptive).  Nothing below is allocated or created before the first adaptive sample pass.
    struct Adaptive {
        float threshold = 0.0f;    // hjr_adaptive.noise_threshold; 0 = off
        uint32_t min_samples = 0;  // as given (0 = two granules; rounded up to the frame's granule at its passes)
        bool frame = false;        // the context's last render was an adaptive sample pass: the fields below describe its frame
        uint32_t owned = 0, last_end = 0;
        uint64_t samples = 0;      // 64 x samples handed to active tiles so far (known on the host: active tiles at launch x pass length)
        DevBuf state, list;        // [owned tile] uint32 n_tile (0 = active) + 1 counter | compacted tile list
        uint32_t* h_active = nullptr; // pinned: tiles still active after the last pass, valid once `ready` has happened
        hipEvent_t ready = nullptr;
    } ad;
    // Temporal accumulation (option "denoise_temporal", csrc/hjr_temporal.hip.h).  Nothing here is allocated before the first render with the
    // option on.  Two slots in rotation: slot[cur] receives the frame being rendered, slot[cur ^ 1] holds the committed previous frame (if have_prev).
    struct Temporal {
        struct Slot {
            hjr_camera cam;
            DevBuf color, variance, history, gbuf, xf; // accumulated unfiltered colour | its variance | h | G-buffer | [M | M^-1] of that render
            DevBuf moments;                            // option "denoise_temporal_moments": float2 (m1, m2) per pixel
        } slot[2];
        DevBuf response;                               // option "denoise_temporal_response": lambda per pixel of the last accumulation
        DevBuf prior;                                  // option "adaptive_temporal": float4 (lp, vp, al, 0) per pixel of the frame being rendered in sample passes
        bool have_prior = false;                       // ... written at that frame's first pass against slot[prior_cur ^ 1]
        int prior_cur = 0;
        bool have_prev = false;
        int cur = 0;
        uint32_t width = 0, height = 0, n_instances = 0; // of the previous frame
        int mode = 0;
    } tmp;
    hjr::Options opt; // hjr_set_option (host/options.hpp): the library reads no environment variable
    // Deforming meshes (hjr_update_vertices, hjr_set_morph, hjr_set_morph_weights).  Kept behind everything else, so that no
    // field the render units read moves.  `gen` counts the geometry: frame data is "unchanged" only when it was built from the current one.
    struct Deform {
        hjr::Morph morph;              // hjr_set_morph's copy; morph.weights: as last set
        uint64_t gen = 0;              // bumped by every call that changes the base, the sets or the weights
        uint64_t built_gen = 0;        // of the current frame data
        uint64_t prep_gen = 0;         // of the prepared frame
        std::vector<float> prep_w;     // device builder: the weights the prepared frame's light table was blended with; its commit blends with them
        uint32_t prep_vertices = 0;    // host builder: vertices the prepare blended
        std::vector<float> vert, norm; // host builder: the working copy build_frame reads (empty without a morph)
        hjr::DeviceMorph dev;          // device builder: deltas, weights and working arrays
    } deform;
};

// One render launch as hjr_render.hip::plan_launch decided it: all but the occupancy query and the buffers sized by the grid
struct LaunchPlan {
    KParams kp;                    // the caller's parameters with the traversal tuning and the stack split of this launch
    bool wf = false;               // wavefront kernel (hjr_wavefront.hip.h), else megakernel (hjr_kernel.hip.h)
    int lds_mode = 0;              // 0 = BVH4 read from memory, 1 = BVH2 staged in LDS with 32-bit stack entries, 2 = with 16-bit entries, 3 = BVH2 from memory
    int var = 0;                   // VAR of the kernel: 2 textures / sky texture, 1 albedo / normal AOVs, 0 colour only
    bool wf_spill = true;          // wavefront kernel: stacks overflow to HBM (SP = false: whole stacks in LDS)
    uint32_t block = HJR_BLOCK;    // threads per workgroup
    int per_cu = 1;                // workgroups per CU; 0 = what the occupancy query admits
    size_t smem = 0;               // dynamic LDS bytes
    bool set_smem = true;          // raise the kernel's dynamic-LDS limit to smem
    bool spill_buf = true;         // reserve d_spill for the stack entries beyond kp.stack_lds_entries
    bool window = false;           // the launch renders a window: the WIN instantiations, which carry its origin (kp.win_word); single chunks
};
