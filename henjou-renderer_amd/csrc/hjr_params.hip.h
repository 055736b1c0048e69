// Kernel parameter block of the Henjou hot path: the scalar part of the reference's Params (kernel/Params.h, filled at
// renderer/renderer.h:1175-1227) plus the device arrays of the flattened scene (csrc/hjr_layout.h).
#pragma once
#include <type_traits>

#include "hjr_layout.h"
#include "hjr_math.hip.h"

struct KParams {
    const float4* nodes;
    const float4* tri_geom;
    const float4* tri_shade;
    const uint32_t* tri_inst;
    const float4* materials;
    const float4* lights;
    const uchar4* lut;
    const uchar4* texels;    // RGBA8 atlas of all material textures
    const uint4* tex_desc;   // per texture slot: (texel offset, width, height, srgb)
    const float* srgb_lut;   // 256-entry sRGB -> linear table (host-computed)
    const float4* sky_tex;   // equirect IBL (float4), null = constant sky
    float4* aov_color;
    float4* aov_albedo;
    float4* aov_normal;
    unsigned int* queue_head;
    unsigned long long* stats;
    unsigned long long* nan_list;    // counting launches: [0] NaN / Inf samples seen, [1 ..] the first HJR_NAN_LIST of them as x | y << 13 | sample << 26
    int lut_w, lut_h;
    int sky_w, sky_h;
    uint32_t n_lights;
    uint32_t width, height, spp, frame, seed, integrator; // width, height: the FULL frame's, also under a render window (work_w / work_h below)
    uint32_t tiles_x, n_owned_items; // items of the launch's queue: owned tiles * pass_chunks * 64 single chunks, fewer when the megakernel groups them (hjr_item_count)
    uint32_t rank, world;
    uint32_t packed;                 // HJR_FLAG_PACKED: the AOV buffers hold this rank's tiles only, [owned tile][64] float4
    uint32_t chunk_spp, n_chunks;    // samples per work item, work items per pixel (hjr_chunking)
    uint32_t n_node_f4, n_tri_f4;    // float4 counts of nodes[] / tri_geom[] (LDS staging)
    uint32_t n_mat_f4, n_light_f4;   // float4 counts of materials[] / lights[] (staged behind the triangles in the LDS variant)
    uint32_t stack_depth;            // traversal stack entries per lane (BVH depth + 1)
    uint32_t* stack_spill;           // memory-path kernels: overflow of the short LDS stacks, [level][lane]
    const uint32_t* tile_order;      // owned tiles, expensive first (hjr_classify_tiles_kernel); null = plain round-robin order
    uint32_t* tile_order_w;          // the same buffer, writable (pre-pass kernels)
    uint32_t* tile_class;            // per owned tile: costliest first hit of its pixel centres: 0 background / light, 1 Disney, 2 metallic (msGGX), 3 glass
    uint32_t* tile_count;            // [0..3] tiles per class, [4..7] scatter cursors
    uint32_t n_owned_tiles;
    uint32_t* tile_bucket;           // per owned tile: sort key of the measured-cost order
    uint32_t* tile_cost;             // per owned tile: closest-hit rays traced for it this frame (feeds the next frame's tile order)
    uint32_t* cost_hist;             // [0..63] tiles per cost bucket, [64..127] scatter cursors
    uint32_t cost_div;               // 64 * samples of the launch that measured tile_cost: rays per tile at one ray per sample
    uint32_t spill_stride;           // lanes in the grid
    uint32_t n_top_nodes;            // memory-path megakernel, BVH4: nodes [0, n_top_nodes) are also staged in LDS by every workgroup (0: none)
    uint32_t stack_lds_entries;      // memory-path kernels: stack entries per lane kept in LDS (the rest overflow to stack_spill)
    uint32_t node_min;               // descent loop of the fused traversals: lanes still holding an inner node below which a pass moves on to the leaves (hjr_traverse.hip.h); always >= 1 (option "node_min" is 1 .. 64, the layout's default otherwise): traverse_fused's loop test relies on it
    uint32_t hold_min, hold_age;     // megakernel: hits of the rare material class wait until a wave has hold_min of them or one has waited hold_age rounds (0: off)
    float4* wf_ctx;                  // wavefront kernel: context records, [workgroup][wf_cap] x 128 bytes (hjr_wavefront.hip.h)
    float4* wf_aov;                  // wavefront kernel, albedo / normal launches: per-context AOV sums, [workgroup][wf_cap] x 32 bytes
    uint32_t wf_cap;                 // contexts per workgroup (power of two, <= 32768: ids travel as uint16 + 1)
    uint32_t wf_refill, wf_trace_min; // trace-stage hand-over threshold (lanes without a ray) / scheduler preference for TRACE (queued rays)
    uint32_t wf_prefetch_min;        // trace-stage hand-over threshold (lanes that have used up their prefetched context)
    float4* part_color;              // [n_chunks][owned tile][64] chunk sums when n_chunks > 1, as the render kernels address them; a sample pass
                                     // allocates its own chunks only and passes the buffer minus chunk0 chunks (only chunks >= chunk0 are stored)
    float4* part_albedo;
    float4* part_normal;
    float cam_pos[3], cam_dir[3], cam_up[3], cam_right[3];
    float cam_f;
    float sky[3]; // scene_sky_default * ibl_intensity
    float ibl_intensity;
    // sample pass (hjr_params.sample_begin / sample_end): the launch renders chunks [chunk0, chunk0 + pass_chunks) of the
    // frame's n_chunks (0 / n_chunks for a whole frame); the buffers behind part_* hold those chunks only
    uint32_t chunk0, pass_chunks;
    // megakernel: a work item is one pixel's group of item_chunks consecutive chunks (a power of two that divides pass_chunks; hjr_layout.h:
    // hjr_item_range).  The wavefront kernels run single chunks: 1 there
    uint32_t item_chunks;
    float4* run_color;              // hjr_finalize_kernel<PASS>: running sums of the frame's earlier passes, [owned tile][64] float4 per AOV
    float4* run_albedo;
    float4* run_normal;
    uint32_t run_load, run_store;    // 1: the running sums hold earlier passes (else they start at +0.0f) / are written back (not the last pass)
    uint32_t sample_end;             // the mean is running sum * (1 / sample_end)
    float2* stat;                    // hjr_finalize_kernel<PASS, ADAPTIVE || VAR>: per owned pixel (S1, S2) over the full chunks received so far,
                                     // [owned tile][64]; null unless the launch is an adaptive sample pass or a sample pass with the variance AOV
    // adaptive sampling (hjr_set_adaptive): all null / 0 unless the launch is an adaptive sample pass
    uint32_t* ad_state;              // per owned tile: 0 = active, else n_tile (the sample_end the tile stopped at); word [n_owned_tiles] counts
                                     // the tiles still active after the pass (zeroed before hjr_finalize_kernel, read back by the host)
    const uint32_t* ad_src;          // hjr_filter_tiles_kernel: the launch's tile order (null = plain round-robin order) ...
    uint32_t* ad_list;               // ... and its stable compaction to the active tiles, which becomes tile_order
    float ad_threshold;              // noise_threshold
    uint32_t ad_decide;              // 1: a stop decision is taken after this pass (sample_end < spp, >= min_samples, >= 2 chunks)
    // render window (DESIGN.md §4 rule 12; hjr_params_window.window): ray generation and the RNG key use the FULL frame's width / height (above) and
    // full-frame pixel coordinates, so a window is the crop of the frame; everything else works on the work rectangle's own tile grid.  The render
    // kernels of a window launch (template parameter WIN) read the three words below cold, next to the other cold parameters of an item's start and
    // end; the kernels of whole-frame launches do not read them at all
    uint32_t work_w, work_h;         // extent of the launch's work rectangle, the window or else the frame: the tile grid (tiles_x) and every output are this size
    uint32_t win_word;               // x0 | y0 << 13, the window's origin (multiples of HJR_TILE) as a WIN kernel adds it to an item word; 0 without a window
};

// Launch parameters that only the start and the end of a work item need (tile list, queue head, output and chunk-sum pointers, shard
// geometry) are read from the kernel-argument segment WHERE they are used instead of living in SGPRs for the whole kernel: the render
// loop keeps ~100 scalar values alive, and every one of these that stays resident pushes another into a VGPR lane (v_writelane at entry,
// v_readlane at each use: VALU instructions inside the round loop).  The empty asm makes the base pointer opaque, so the compiler can
// neither hoist the load out of the loop nor merge it with the by-value copy of P.
template <typename T> HD T cold_param(size_t offset)
{
    const char __attribute__((address_space(4)))* ka = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *reinterpret_cast<const T __attribute__((address_space(4)))*>(ka + offset);
}
#define HJR_COLD(field) cold_param<decltype(KParams::field)>(offsetof(KParams, field))
