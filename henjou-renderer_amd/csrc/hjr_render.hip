// The render path of libhenjou_hip.so: launch plan, pass rules of a progressive frame, kernel parameters, tile order, the render kernel and what runs behind it (chunk sums ->
// pixel means, both firefly rules, adaptive sampling and its rule 11), and the hjr_render* entry points.  Replaces the reference's Params fill + optixLaunch (renderer/renderer.h:1175-1242).
#include "hjr_device_internal.h"
#include "hjr_aux.hip.h"

// the render kernels live in their own translation units, which instantiate these (hjr_launch.hip.h: this unit does not see it)
template <int I, bool S> int hjr_launch(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t); // hjr_launch_{nee,pt,mis}.hip
template <int I> int hjr_launch_fast(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);    // hjr_launch_fast_{nee,pt}.hip (HJR_FLAG_FAST_MATH)

// descent loops of the fused traversals (hjr_traverse.hip.h): lanes still descending below which a pass moves on to the leaves
#ifndef HJR_NODE_MIN_LDS
#define HJR_NODE_MIN_LDS 6     /* megakernel, LDS-resident scenes (round 2, with AOVs, 1 / 4 / 8 / 12 / 16: 139.8 / 128.9 / 129.8 / 135.2 / 140.4 ms; round 3 with a carry-over of 14 lanes, 4 / 5 / 6 / 7 / 8: 110.1 / 109.6 / 109.15 / 109.05 / 109.3) */
#endif
#ifndef HJR_NODE_MIN_LDS_WF
#define HJR_NODE_MIN_LDS_WF 8  /* wavefront kernel, LDS-resident scenes (1 / 4 / 8 / 12 / 16: 132.4 / 125.4 / 124.8 / 125.7 / 126.4 ms) */
#endif
#ifndef HJR_NODE_MIN_MEM
#define HJR_NODE_MIN_MEM 24    /* scenes read from memory (1 M triangles, 1 / 8 / 16 / 24 / 32: megakernel 280 / 197 / 180 / 179 / 190 ms, wavefront 255 / 213 / 194 / 189 / 192) */
#endif
#ifndef HJR_TOP_NODES
#define HJR_TOP_NODES 85 /* memory layouts, BVH4: nodes of the top of the tree (levels 0 - 3) staged in LDS per workgroup (option "top_nodes"; 1 M triangles, 0 / 21 / 85 / 140 / 200 / 341: 166.9 / 165.9 / 164.6 / 164.5 / 164.6 / 273.7 ms — the last one loses a workgroup per CU) */
#endif
#ifndef HJR_HOLD_MIN
#define HJR_HOLD_MIN 8 /* megakernel: lanes of the rare material class (multiple-scattering GGX) a wave collects before it shades them (0: never hold; C2 with AOVs, 0 / 4 / 8 / 16 / 32: 129.0 / 126.5 / 126.2 / 127.9 / 144.2 ms) */
#endif
#ifndef HJR_ITEM_CHUNKS
#define HJR_ITEM_CHUNKS 2 /* long single-GPU megakernel launches: chunks of a pixel per work item (option "item_chunks"; launch_render) */
#endif
#ifndef HJR_ITEM_GROUP_MIN
#define HJR_ITEM_GROUP_MIN 192u /* ... "long": single-chunk items per lane of a full grid from which the chunks are grouped */
#endif
#ifndef HJR_HOLD_AGE
#define HJR_HOLD_AGE 2 /* ... or rounds the oldest of them has waited */
#endif

// Kernel family, layout, variant, grid shape, LDS split and traversal tuning of one render launch.  `fast`: an approximate-arithmetic
// launch (hjr_launch_fast_*.hip hold the megakernel family only).
LaunchPlan hjr::plan_launch(const hjr_ctx* c, const KParams& kp, uint64_t n_items, int lds_mode, int integrator, bool fast)
{
    LaunchPlan pl;
    pl.kp = kp; pl.lds_mode = lds_mode;
    // the albedo / normal AOV sums cost 6 VGPRs per lane: a separate variant for callers that only want aov_color
    pl.var = (kp.tex_desc || kp.sky_tex) ? 2 : ((kp.aov_albedo || kp.aov_normal) ? 1 : 0);
    const bool lds_layout = lds_mode == 1 || lds_mode == 2;
    const size_t scene_bytes = ((size_t)kp.n_node_f4 + kp.n_tri_f4 + kp.n_mat_f4 + kp.n_light_f4) * 16;
    const uint32_t short_stack = (uint32_t)c->opt.get(hjr::OPT_SHORT_STACK, HJR_SHORT_STACK); // tests force the overflow path with 2
    // Two kernel families produce the same bits (hjr_kernel.hip.h / hjr_wavefront.hip.h); which one is faster depends on the launch
    // (MI355X, profiles/r02_experiments.md §4).  Bundled scene (LDS-resident), 1080p x 256 spp: MIS 193 ms wavefront vs 234 ms megakernel
    // (the NEE shadow ray and the next closest-hit ray of its bounce are traced by sorted, full waves), NEE colour-only 126.7 vs 126.6,
    // NEE with albedo / normal AOVs 145.7 vs 128.9, Pathtrace 104.7 vs 91.2.  Scenes read from memory (1 M triangles, 1080p x 64 spp):
    // MIS 416 vs 635 ms, NEE 188 vs 179.  So: MIS -> wavefront kernel, everything else -> megakernel.  option "pipeline" overrides.
    const int pe = c->opt.get(hjr::OPT_PIPELINE, 0); // option "pipeline": 1 megakernel, 2 wavefront kernel
    bool wf = integrator == HJR_INTEGRATOR_MIS;
    if (pe) wf = pe == 2;
    // the wavefront kernel's queue positions are free-running 32-bit counters per workgroup (hjr_wavefront.hip.h::WfShared): a context is
    // queued at most ~12 times per sample; frames that could bring one workgroup near 2^32 pushes (4x its even share) stay with the megakernel
    if ((double)n_items * kp.chunk_spp * 12.0 * 4.0 / (double)(c->n_cus > 0 ? c->n_cus : 1) >= 4.0e9) wf = false;
#ifdef HJR_LEAN_VARIANT /* kernel experiments (make variant X="-DHJR_LEAN_VARIANT ..."): only the megakernel is instantiated: builds in seconds */
    wf = false;
#endif
    if (wf && !fast) {
        // Workgroup-local wavefront kernel (hjr_wavefront.hip.h): one 1024-thread workgroup per CU for every layout.  LDS holds the top of
        // the traversal stacks, the scene tables (LDS layouts), the queue header, the hit slots and the id rings; what is left after the
        // fixed parts decides how many stack entries per lane stay in LDS (the rest overflows to HBM).
        uint32_t cap = lds_layout ? 2048 : 4096; // contexts per workgroup: more of them in flight pay when every node comes from memory (1 M triangles: 272 -> 259 ms)
        { const int v = c->opt.get(hjr::OPT_WF_CAP, (int)cap); if ((v & (v - 1)) == 0) cap = (uint32_t)v; }
        const size_t fixed = (lds_layout ? scene_bytes : 0) + 96 + (size_t)HJR_WF_QUEUES * cap * 2;
        const size_t lds_max = 160u * 1024u;
        if (fixed + (size_t)HJR_BLOCK_LDS * 4 * 4 <= lds_max) { // at least four stack entries per lane fit; otherwise: megakernel
            uint32_t lds_entries = std::min<uint32_t>((uint32_t)((lds_max - fixed) / ((size_t)HJR_BLOCK_LDS * 4)), kp.stack_depth);
            if ((!lds_layout || c->opt.is_set(hjr::OPT_SHORT_STACK)) && lds_entries > short_stack) lds_entries = short_stack;
            pl.wf = true; pl.block = HJR_BLOCK_LDS;
            pl.wf_spill = !(lds_layout && lds_entries >= kp.stack_depth); // false: whole stacks in LDS
            pl.smem = (size_t)HJR_BLOCK_LDS * lds_entries * 4 + fixed;
            pl.kp.wf_cap = cap; pl.kp.stack_lds_entries = lds_entries;
            pl.kp.wf_refill = (uint32_t)c->opt.get(hjr::OPT_WF_REFILL, HJR_WF_REFILL); // tuning options
            pl.kp.wf_trace_min = (uint32_t)c->opt.get(hjr::OPT_WF_TRACE_MIN, HJR_WF_TRACE_MIN); pl.kp.wf_prefetch_min = (uint32_t)c->opt.get(hjr::OPT_WF_PREFETCH_MIN, HJR_WF_PREFETCH_MIN);
        }
    }
    pl.kp.hold_min = (uint32_t)c->opt.get(hjr::OPT_HOLD_MIN, HJR_HOLD_MIN); pl.kp.hold_age = (uint32_t)c->opt.get(hjr::OPT_HOLD_AGE, HJR_HOLD_AGE); // tuning options
    const uint32_t nm_forced = (uint32_t)c->opt.get(hjr::OPT_NODE_MIN, 0); // option "node_min"
    pl.kp.node_min = nm_forced ? nm_forced : (lds_layout ? (pl.wf ? HJR_NODE_MIN_LDS_WF : HJR_NODE_MIN_LDS) : HJR_NODE_MIN_MEM);
    if (pl.wf) return pl;
    if (lds_layout) { // megakernel, BVH2 + tables staged in LDS: one workgroup per CU, whole stacks in LDS
        pl.block = HJR_BLOCK_LDS; pl.spill_buf = false;
        pl.smem = (((size_t)HJR_BLOCK_LDS * kp.stack_depth * (lds_mode == 2 ? 2 : 4) + 15) / 16) * 16 + scene_bytes;
        return pl;
    }
    // megakernel, scene read from memory: short stacks in LDS, BVH4 with the top of the tree (breadth-first ids: the first nodes) next to
    // them, sized so that four workgroups still share a CU
    const uint32_t lds_entries = std::min<uint32_t>(kp.stack_depth, short_stack);
    const uint32_t n_top = lds_mode == 0 ? std::min<uint32_t>((uint32_t)c->opt.get(hjr::OPT_TOP_NODES, HJR_TOP_NODES), kp.n_node_f4 / HJR_NODE4_F4) : 0u;
    pl.smem = (((size_t)HJR_BLOCK * lds_entries * 4 + 15) / 16) * 16 + (size_t)n_top * HJR_NODE4_F4 * 16;
    pl.set_smem = pl.smem > 48 * 1024;
    pl.per_cu = c->opt.is_set(hjr::OPT_BLOCKS_PER_CU) ? c->opt.get(hjr::OPT_BLOCKS_PER_CU, 0) : 0;
    pl.kp.stack_lds_entries = lds_entries; pl.kp.n_top_nodes = n_top;
    return pl;
}

static const uint32_t PASS_FLAGS = HJR_FLAG_PACKED | HJR_FLAG_ZERO_UNOWNED | HJR_FLAG_FAST_MATH; // the flags that change pixels
// options "firefly_clamp" > 0 and "firefly_clamp_passes" 1 (DESIGN.md §4 rule 10): a progressive frame keeps the colour chunk sums of all its passes
bool hjr::firefly_keeps_chunks(const hjr_ctx* c) { return c->opt.get(hjr::OPT_FIREFLY_CLAMP, 0) > 0 && c->opt.get(hjr::OPT_FIREFLY_CLAMP_PASSES, 0) == 1; }

// The pass rules, checked before a call enqueues or writes anything: HJR_ERR_ARG for a bad range, HJR_ERR_STATE for a pass that does not
// continue the context's progressive frame.  Changes nothing; end_pass records a launch once it is enqueued.
int hjr::check_pass(const hjr_ctx* c, const ParamsW* p, uint32_t aovs, PassRange& r)
{
    r = PassRange();
    r.aovs = aovs;
    if (p->sample_end == 0) {
        if (p->sample_begin != 0) { set_error("hjr_render: sample_begin without sample_end (sample_end 0 renders the whole frame)"); return HJR_ERR_ARG; }
        return HJR_OK;
    }
    if (p->spp == 0) { set_error("hjr_render: width, height and spp must be positive"); return HJR_ERR_ARG; }
    if (p->sample_begin == 0 && p->sample_end == p->spp) return HJR_OK; // the whole frame, through the same path
    if (c->opt.get(hjr::OPT_FIREFLY_CLAMP, 0) > 0 && !hjr::firefly_keeps_chunks(c)) { // the rule needs every chunk sum of a pixel; a progressive frame keeps running sums only
        set_error("hjr_render: option \"firefly_clamp\" takes whole-frame renders only: sample pass [" + std::to_string(p->sample_begin) + ", " + std::to_string(p->sample_end) +
                  ") of " + std::to_string(p->spp) + " spp refused");
        return HJR_ERR_ARG;
    }
    const uint32_t g = hjr_chunk_spp(p->spp);
    if (p->sample_begin >= p->sample_end || p->sample_end > p->spp) {
        set_error("hjr_render: sample pass [" + std::to_string(p->sample_begin) + ", " + std::to_string(p->sample_end) + ") is not a range inside [0, spp = " + std::to_string(p->spp) + "]");
        return HJR_ERR_ARG;
    }
    if (hjr_n_chunks(p->spp) == 1) { set_error("hjr_render: a frame of " + std::to_string(p->spp) + " spp is a single chunk: only the whole range [0, spp) is a pass"); return HJR_ERR_ARG; }
    if (p->sample_begin % g || (p->sample_end % g && p->sample_end != p->spp)) {
        set_error("hjr_render: sample pass boundaries must be multiples of hjr_sample_granule(" + std::to_string(p->spp) + ") = " + std::to_string(g) + " or equal spp");
        return HJR_ERR_ARG;
    }
    r.pass = true; r.begin = p->sample_begin; r.end = p->sample_end;
    if (r.begin == 0) return HJR_OK; // starts a progressive frame (replacing an unfinished one)
    const hjr_ctx::PassSession& s = c->pass;
    std::string bad;
    if (!s.active) bad = s.committed ? "the frame ended when its last active tile stopped and option \"adaptive_temporal\" committed its history (the next pass starts a new frame at sample 0)"
                                     : "no progressive frame is open (its first pass starts at sample 0)";
    else if (r.begin != s.next) bad = "sample_begin " + std::to_string(r.begin) + " does not continue the previous pass, which ended at " + std::to_string(s.next);
    else if (p->width != s.p.width || p->height != s.p.height) bad = "width / height differ from the frame's first pass";
    else if (memcmp(p->window, s.p.window, sizeof(p->window)) != 0) bad = "window differs from the frame's first pass";
    else if (p->spp != s.p.spp) bad = "spp differs from the frame's first pass";
    else if (p->frame != s.p.frame) bad = "frame differs from the frame's first pass";
    else if (p->seed != s.p.seed) bad = "seed differs from the frame's first pass";
    else if (p->integrator != s.p.integrator) bad = "integrator differs from the frame's first pass";
    else if (memcmp(&p->camera, &s.p.camera, sizeof(hjr_camera)) != 0) bad = "camera differs from the frame's first pass";
    else if (memcmp(p->sky, s.p.sky, sizeof(p->sky)) != 0 || memcmp(&p->ibl_intensity, &s.p.ibl_intensity, sizeof(float)) != 0) bad = "sky / ibl_intensity differ from the frame's first pass";
    else if (p->rank != s.p.rank || p->world_size != s.p.world_size) bad = "rank / world_size differ from the frame's first pass";
    else if ((p->flags & PASS_FLAGS) != (s.p.flags & PASS_FLAGS)) bad = "flags PACKED / ZERO_UNOWNED / FAST_MATH differ from the frame's first pass";
    else if (aovs != s.aovs) bad = "the set of AOVs differs from the frame's first pass";
    else if (c->frame_gen != s.gen) bad = "the frame data changed since the frame's first pass (scene, transforms, LUT or sky)";
    if (!bad.empty()) { set_error("hjr_render: sample pass [" + std::to_string(r.begin) + ", " + std::to_string(r.end) + ") refused: " + bad); return HJR_ERR_STATE; }
    return HJR_OK;
}
// after a launch was enqueued: the progressive frame goes on to r.end, or ends (last pass, or a whole-frame render)
static void end_pass(hjr_ctx* c, const ParamsW* p, const PassRange& r)
{
    hjr_ctx::PassSession& s = c->pass;
    s.committed = false;
    if (!r.pass || r.end == p->spp) { s.active = false; return; }
    if (r.begin == 0) { s.p = *p; s.aovs = r.aovs; s.gen = c->frame_gen; }
    s.active = true;
    s.next = r.end;
}

// argument checks and tile geometry
int hjr::frame_geometry(const hjr_ctx* c, const ParamsW* p, const void* d_color, const PassRange& pr, FrameGeom& g)
{
    if (!c || !p || !d_color) { set_error("hjr_render: null argument"); return HJR_ERR_ARG; }
    if (!c->have_scene || !c->have_frame) { set_error("hjr_render: upload a scene and set transforms first"); return HJR_ERR_STATE; }
    if (p->width == 0 || p->height == 0 || p->spp == 0) { set_error("hjr_render: width, height and spp must be positive"); return HJR_ERR_ARG; }
    if (p->width > 8192 || p->height > 8192) { set_error("hjr_render: frames larger than 8192 x 8192 are not supported"); return HJR_ERR_ARG; }
    if (p->integrator > HJR_INTEGRATOR_MIS) { set_error("hjr_render: unknown integrator"); return HJR_ERR_ARG; }
    g.world = p->world_size ? p->world_size : 1u;
    if (p->rank >= g.world) { set_error("hjr_render: rank >= world_size"); return HJR_ERR_ARG; }
    if (const int rc = work_rect(p, "hjr_render", g.rect)) return rc;
    if (g.rect.window && c->opt.get(hjr::OPT_ADAPTIVE_TEMPORAL, 0) != 0) { set_error("hjr_render: a render window (hjr_params_window.window) cannot be combined with option \"adaptive_temporal\" (its prior is a whole-frame gather)"); return HJR_ERR_ARG; }
    g.tiles_x = (g.rect.w + HJR_TILE - 1) / HJR_TILE;
    const uint64_t n_tiles = (uint64_t)g.tiles_x * ((g.rect.h + HJR_TILE - 1) / HJR_TILE);
    g.owned = (n_tiles > p->rank) ? (n_tiles - p->rank + g.world - 1) / g.world : 0;
    g.chunk_spp = hjr_chunk_spp(p->spp); g.n_chunks = hjr_n_chunks(p->spp);
    g.pr = pr;
    g.chunk0 = pr.pass ? pr.begin / g.chunk_spp : 0u;
    g.pass_chunks = pr.pass ? (pr.end - pr.begin + g.chunk_spp - 1) / g.chunk_spp : g.n_chunks;
    g.n_items = g.owned * g.pass_chunks * 64;
    // the 32-bit queue head overshoots n_items by at most 64 per wave of the persistent grid (every wave stops fetching once it
    // has seen the queue dry, hjr_kernel.hip.h); 2^24 covers 262 144 waves, far more than any resident grid
    if (g.n_items >= 0xffffffffull - (1ull << 24)) { set_error("hjr_render: image too large (more than 2^32 - 2^24 work items per launch)"); return HJR_ERR_ARG; }
    // node format / LDS staging were decided by the host builder for this frame (host/frame.cpp)
    g.lds_mode = launch_layout(c->frame);
    return HJR_OK;
}

// the frame data and scene tables a kernel traverses, and their sizes (LDS staging, stack depth)
void hjr::bind_scene_tables(const hjr_ctx* c, KParams& kp)
{
    kp.nodes = (const float4*)c->d_nodes.p;
    kp.tri_geom = (const float4*)c->d_tri_geom.p;
    kp.tri_shade = (const float4*)c->d_tri_shade.p;
    kp.tri_inst = (const uint32_t*)c->d_tri_inst.p;
    kp.materials = (const float4*)c->d_materials.p;
    kp.lights = (const float4*)c->d_lights.p;
    kp.n_node_f4 = c->frame.n_nodes * (c->frame.width == 2 ? HJR_NODE2_F4 : HJR_NODE4_F4);
    kp.n_tri_f4 = (c->frame.n_tris ? c->frame.n_tris : 1u) * HJR_TRI_F4;
    kp.stack_depth = c->frame.stack_need; // exact worst case for this tree (host/frame.cpp)
    kp.n_mat_f4 = (uint32_t)c->scene.materials.size() * HJR_MAT_F4;
    kp.n_light_f4 = c->frame.n_lights * HJR_LIGHT_F4;
}

// work area, output zeroing, chunk-sum buffers, and the kernel parameters of scene, frame and outputs
static int bind_params(hjr_ctx* c, const ParamsW* p, const FrameGeom& g, void* d_color, void* d_albedo, void* d_normal, void* d_var, hipStream_t st, KParams& kp)
{
    if (c->d_work.cap < WorkArea::BYTES) {
        std::vector<unsigned char> z(WorkArea::BYTES, 0);
        if (!c->d_work.upload(z.data(), WorkArea::BYTES, st)) { set_error("hjr_render: work buffer allocation failed"); return HJR_ERR_DEVICE; }
    }
    HIPCHK(hipMemsetAsync(c->d_work.p, 0, WorkArea::BYTES, st));
    const size_t img_bytes = (size_t)g.rect.w * g.rect.h * 16;
    const bool packed = (p->flags & HJR_FLAG_PACKED) != 0;
    if (!packed && g.world > 1 && (p->flags & HJR_FLAG_ZERO_UNOWNED)) {
        HIPCHK(hipMemsetAsync(d_color, 0, img_bytes, st));
        if (d_albedo) HIPCHK(hipMemsetAsync(d_albedo, 0, img_bytes, st));
        if (d_normal) HIPCHK(hipMemsetAsync(d_normal, 0, img_bytes, st));
        if (d_var) HIPCHK(hipMemsetAsync(d_var, 0, img_bytes / 4, st)); // one float per pixel
    }

    memset(&kp, 0, sizeof(kp));
    kp.n_owned_tiles = (uint32_t)g.owned;
    if (g.n_chunks > 1) {
        // chunk sums of THIS rank's tiles and this launch's chunks only: [chunk - chunk0][owned tile][64] float4 (1/world of the frame;
        // a sample pass needs its own chunks only; allocated once per size)
        // Rule 10 (firefly_keeps_chunks) reads every colour chunk sum of the progressive frame at every pass: the colour buffer then holds all
        // n_chunks, sized by the frame's first pass and not moved by the later ones (the same size), and is addressed from its base.
        const bool keep = g.pr.pass && hjr::firefly_keeps_chunks(c);
        const size_t part_bytes = (size_t)g.owned * 64u * 16u * g.pass_chunks;
        DevBuf* pb[3] = { &c->d_part_color, &c->d_part_albedo, &c->d_part_normal };
        DevBuf* rb[3] = { &c->d_run_color, &c->d_run_albedo, &c->d_run_normal };
        void* want[3] = { d_color, d_albedo, d_normal };
        for (int i = 0; i < 3; i++) {
            if (want[i] && !pb[i]->reserve(i == 0 && keep ? (size_t)g.owned * 64u * 16u * g.n_chunks : part_bytes)) { set_error("hjr_render: chunk-sum buffer allocation failed"); return HJR_ERR_DEVICE; }
            // running sums of a progressive frame, [owned tile][64] float4; the same size for every pass of one frame, so kept across them
            if (want[i] && g.pr.pass && !rb[i]->reserve((size_t)g.owned * 64u * 16u)) { set_error("hjr_render: running-sum buffer allocation failed"); return HJR_ERR_DEVICE; }
        }
        // the render kernels address chunk k at k * owned * 64: a sample pass's buffers start at its first chunk, so the pointers are
        // moved back by chunk0 chunks (no chunk below chunk0 is stored or read; 0 for a one-shot frame)
        const size_t back = (size_t)g.chunk0 * g.owned * 64u;
        kp.part_color = (float4*)c->d_part_color.p - (keep ? 0u : back);
        kp.part_albedo = d_albedo ? (float4*)c->d_part_albedo.p - back : nullptr;
        kp.part_normal = d_normal ? (float4*)c->d_part_normal.p - back : nullptr;
        if (g.pr.pass) {
            kp.run_color = (float4*)c->d_run_color.p;
            kp.run_albedo = d_albedo ? (float4*)c->d_run_albedo.p : nullptr;
            kp.run_normal = d_normal ? (float4*)c->d_run_normal.p : nullptr;
            kp.run_load = g.pr.begin > 0 ? 1u : 0u;
            kp.run_store = g.pr.end < p->spp ? 1u : 0u;
            kp.sample_end = g.pr.end;
        }
    }
    kp.chunk_spp = g.chunk_spp; kp.n_chunks = g.n_chunks;
    kp.chunk0 = g.chunk0; kp.pass_chunks = g.pass_chunks; kp.item_chunks = 1u; // (launch_render groups chunks for the megakernel)
    hjr::bind_scene_tables(c, kp);
    kp.lut = (c->lut_w > 0) ? (const uchar4*)c->d_lut.p : nullptr;
    kp.lut_w = c->lut_w; kp.lut_h = c->lut_h;
    if (c->n_textures) { kp.texels = (const uchar4*)c->d_texels.p; kp.tex_desc = (const uint4*)c->d_tex_desc.p; kp.srgb_lut = (const float*)c->d_srgb_lut.p; }
    if (c->sky_w > 0) { kp.sky_tex = (const float4*)c->d_sky.p; kp.sky_w = c->sky_w; kp.sky_h = c->sky_h; }
    kp.ibl_intensity = p->ibl_intensity;
    kp.aov_color = (float4*)d_color; kp.aov_albedo = (float4*)d_albedo; kp.aov_normal = (float4*)d_normal;
    char* const work = (char*)c->d_work.p;
    kp.queue_head = (unsigned int*)(work + WorkArea::QUEUE_HEAD);
    kp.stats = (unsigned long long*)(work + WorkArea::STATS);
    kp.nan_list = (unsigned long long*)(work + WorkArea::NAN_LIST);
    kp.n_lights = c->frame.n_lights;
    kp.width = p->width; kp.height = p->height; kp.work_w = g.rect.w; kp.work_h = g.rect.h; kp.win_word = g.rect.x0 | (g.rect.y0 << 13);
    kp.spp = p->spp; kp.frame = p->frame; kp.seed = p->seed; kp.integrator = p->integrator;
    kp.tiles_x = g.tiles_x; kp.n_owned_items = (uint32_t)g.n_items;
    kp.rank = p->rank; kp.world = g.world;
    kp.packed = packed ? 1u : 0u;
    for (int k = 0; k < 3; k++) {
        kp.cam_pos[k] = p->camera.pos[k]; kp.cam_dir[k] = p->camera.dir[k];
        kp.cam_up[k] = p->camera.up[k]; kp.cam_right[k] = p->camera.right[k];
        kp.sky[k] = p->sky[k] * p->ibl_intensity; // __miss__ms: texel * params.ibl_intensity
    }
    kp.cam_f = p->camera.f;

    c->stats.lds_mode = (uint32_t)g.lds_mode; c->stats.stack_need = c->frame.stack_need;
    return HJR_OK;
}

// cost-ordered tile list (hjr_classify_tiles_kernel): option "tile_order" = 0 keeps the plain round-robin order
static int order_tiles(hjr_ctx* c, const ParamsW* p, const FrameGeom& g, KParams& kp, hipStream_t st)
{
    const int order_knob = c->opt.get(hjr::OPT_TILE_ORDER, -1); // option "tile_order"
    if (order_knob == 0 || g.owned == 0) return HJR_OK;
    const size_t tb = (size_t)g.owned * 4;
    bool grown = false;
    if (!c->d_tiles.reserve(3 * tb, &grown)) { set_error("hjr_render: tile list allocation failed"); return HJR_ERR_DEVICE; }
    if (grown) c->cost_tag = 0; // the classes of the previous frames went with the buffer
    char* const work = (char*)c->d_work.p;
    kp.tile_order_w = (uint32_t*)c->d_tiles.p;
    kp.tile_class = (uint32_t*)((char*)c->d_tiles.p + tb);
    kp.tile_bucket = (uint32_t*)((char*)c->d_tiles.p + 2 * tb);
    kp.tile_count = (uint32_t*)(work + WorkArea::TILE_COUNT);
    // Inside a class the tiles can also be ordered by what they cost in the previous frame of the same configuration.  That
    // shortens the tail of a launch further (an 8-GPU share of C2: 19.0 -> 18.4 ms) but gives up the scanline order inside a
    // class, which costs 1.6 % when the launch is long (N = 1: 134.6 -> 136.8 ms): used when the frame is split over several
    // GPUs.  Pure scheduling: no pixel depends on it.  Option "tile_order" = 1 / 2 forces it off / on.
    const bool cost_feedback = order_knob == 2 || (order_knob != 1 && g.world > 1);
    const uint64_t tag = ((uint64_t)p->width << 48) ^ ((uint64_t)p->height << 32) ^ ((uint64_t)p->spp << 12) ^ ((uint64_t)g.world << 8) ^
                         ((uint64_t)p->rank << 2) ^ (uint64_t)p->integrator ^ 0x8000000000000000ull;
    bool have_cost = false;
    if (cost_feedback) {
        if (!c->d_tile_cost.reserve(tb, &grown)) { set_error("hjr_render: tile cost allocation failed"); return HJR_ERR_DEVICE; }
        if (grown) c->cost_tag = 0;
        // (the costs and classes are per tile of the work rectangle's grid: those of another window are another configuration)
        have_cost = c->cost_tag == tag && c->cost_rect == g.rect.key();
        if (!have_cost) HIPCHK(hipMemsetAsync(c->d_tile_cost.p, 0, tb, st));
        c->cost_tag = tag; c->cost_rect = g.rect.key();
        kp.tile_cost = (uint32_t*)c->d_tile_cost.p;
        kp.cost_hist = (uint32_t*)(work + WorkArea::COST_HIST);
        // the costs were measured by the previous launch of this configuration: normalised by ITS samples (a whole frame, or the
        // previous sample pass of a progressive frame, whose later passes thus reuse the costs measured by the earlier ones)
        const uint32_t launch_samples = g.pr.pass ? g.pr.end - g.pr.begin : p->spp;
        kp.cost_div = 64u * (have_cost && c->cost_samples ? c->cost_samples : launch_samples);
        c->cost_samples = launch_samples;
    }
    const unsigned tg = (unsigned)((g.owned + 255) / 256);
    if (have_cost) {
        hipLaunchKernelGGL(hjr_cost_hist_kernel, dim3(tg), dim3(256), 0, st, kp);
        hipLaunchKernelGGL(hjr_cost_scatter_kernel, dim3(tg), dim3(256), 0, st, kp);
    } else {
        const unsigned cg = (unsigned)std::min<uint64_t>(g.owned, (uint64_t)c->n_cus * 16);
        const size_t csm = (size_t)64 * kp.stack_depth * 4;
        if (c->frame.width == 2) hipLaunchKernelGGL(hjr_classify_tiles_kernel<2>, dim3(cg), dim3(64), csm, st, kp);
        else hipLaunchKernelGGL(hjr_classify_tiles_kernel<4>, dim3(cg), dim3(64), csm, st, kp);
        hipLaunchKernelGGL(hjr_order_tiles_kernel, dim3(tg), dim3(256), 0, st, kp);
    }
    HIPCHK(hipGetLastError());
    kp.tile_order = (const uint32_t*)c->d_tiles.p;
    return HJR_OK;
}

// the render kernel
static int launch_render(hjr_ctx* c, const ParamsW* p, const FrameGeom& g, const KParams& kp, hipStream_t st)
{
    const bool stats = (p->flags & HJR_FLAG_STATS) != 0;
    bool fast = false;
#ifdef HJR_HAVE_FAST
    // approximate-arithmetic kernels (megakernel family).  A counting launch stays exact, and so does MIS: its exact launch runs on the
    // wavefront kernels, which beat the approximate megakernel (C2: 175 vs 185 ms), so the flag would only make it slower
    fast = (p->flags & HJR_FLAG_FAST_MATH) && !stats && p->integrator != HJR_INTEGRATOR_MIS;
#endif
    LaunchPlan pl = hjr::plan_launch(c, kp, g.n_items, g.lds_mode, p->integrator, fast);
    pl.window = g.rect.window; // the kernels that carry the window's origin; every whole-frame launch runs the kernels it always ran
    // Megakernel: a work item is a pixel's group of r consecutive chunks (hjr_layout.h: hjr_item_range), r = the largest power of two <=
    // option "item_chunks" that divides the launch's chunk count.  The queue then holds 1 / r of the single-chunk items frame_geometry
    // counted, and its head still overshoots by at most 64 per wave, so the margin taken there covers every r.
    // Default (MI355X, profiles/item_chunks.json): longer items save a lane the item-end work and the idle round behind an item, a share of
    // the launch, and add a cost that grows with the item's length and not with the launch's.  1080p, bundled scene, kernel ms with single
    // chunks -> pairs: 256 spp 108.9 -> 107.3, 192 spp 82.2 -> 82.0, 128 spp 55.5 -> 56.2, 96 spp 42.4 -> 43.7; groups of 4 / 8 chunks lose at
    // every length measured.  So: pairs when a lane of the full grid has at least HJR_ITEM_GROUP_MIN single-chunk items to go through
    // (253 at 256 spp, 190 at 192), else single chunks.  The threshold rests on this one scene at this one resolution, and the
    // difference at 192 spp is inside the run-to-run spread: between the loss at 127 items per lane and the gain at 253 it is an
    // interpolation.  Single chunks for a rank of a shard (an 8-GPU share took 19.0 ms with 8-sample runs against 21.0 ms with 16) and for
    // counting launches, and for frames of more than 512 spp, whose chunks are 16 samples and longer: a pair of those is as long as four
    // 8-sample chunks, and at 1024 spp pairs measured 412.3 against 411.7 ms.  A launch of single chunks runs the SINGLE instantiation of its kernel, which does not carry the item rule.
    uint64_t n_items = g.n_items;
    if (!pl.wf && p->integrator != HJR_INTEGRATOR_MIS) { // (MIS runs the wavefront kernels; its megakernel, an option, keeps single chunks)
        const bool is_long = g.n_items >= (uint64_t)(c->n_cus > 0 ? c->n_cus : 1) * HJR_BLOCK_LDS * HJR_ITEM_GROUP_MIN;
        const int def = (g.world > 1 || stats || !is_long || g.chunk_spp > 8u) ? 1 : HJR_ITEM_CHUNKS;
        pl.kp.item_chunks = g.rect.window ? 1u : hjr_item_chunks((uint32_t)c->opt.get(hjr::OPT_ITEM_CHUNKS, def), g.pass_chunks); // (a window: single chunks, the only form its kernels have)
        n_items = hjr_item_count(g.n_items / ((uint64_t)g.pass_chunks * 64u), g.pass_chunks, pl.kp.item_chunks); // (g.n_items counts the active tiles of an adaptive pass)
        pl.kp.n_owned_items = (uint32_t)n_items;
    }
    c->stats.item_chunks = pl.kp.item_chunks;
    c->stats.pipeline = pl.wf ? 1u : 0u; c->stats.fast_math = fast ? 1u : 0u; c->stats.stack_lds_entries = pl.kp.stack_lds_entries;
    using LaunchFn = int (*)(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
#ifdef HJR_LEAN_VARIANT
    LaunchFn fn = hjr_launch<HJR_INTEGRATOR_NEE, false>;
#else
    static const LaunchFn exact[6] = { hjr_launch<HJR_INTEGRATOR_NEE, false>, hjr_launch<HJR_INTEGRATOR_NEE, true>, hjr_launch<HJR_INTEGRATOR_PT, false>,
                                       hjr_launch<HJR_INTEGRATOR_PT, true>, hjr_launch<HJR_INTEGRATOR_MIS, false>, hjr_launch<HJR_INTEGRATOR_MIS, true> };
    LaunchFn fn = exact[p->integrator * 2 + (stats ? 1 : 0)];
#ifdef HJR_HAVE_FAST
    if (fast) fn = p->integrator == HJR_INTEGRATOR_NEE ? hjr_launch_fast<HJR_INTEGRATOR_NEE> : hjr_launch_fast<HJR_INTEGRATOR_PT>;
#endif
#endif
    if (const int rc = fn(c, pl, n_items, st)) return rc;
    return launched();
}

// An adaptive sample pass (hjr_set_adaptive), before bind_params: the tiles still active size the launch.  A continuing
// pass waits here for the count the previous pass of its frame read back (4 bytes, pinned).  The first adaptive pass of a context creates
// the event and the pinned word.
static int adaptive_items(hjr_ctx* c, FrameGeom& g, uint32_t& active)
{
    hjr_ctx::Adaptive& ad = c->ad;
    if (!ad.ready) HIPCHK(hipEventCreateWithFlags(&ad.ready, hipEventDisableTiming));
    if (!ad.h_active) HIPCHK(hipHostMalloc((void**)&ad.h_active, sizeof(uint32_t), hipHostMallocDefault));
    active = (uint32_t)g.owned;
    if (g.pr.begin > 0) {
        if (!ad.frame || ad.owned != (uint32_t)g.owned) { set_error("hjr_render: the progressive frame has no adaptive state"); return HJR_ERR_STATE; }
        HIPCHK(hipEventSynchronize(ad.ready));
        active = *ad.h_active;
    }
    g.n_items = (uint64_t)active * g.pass_chunks * 64; // the render kernels' queue holds the active tiles only
    return HJR_OK;
}
// ... after bind_params: the tile states (+ the counter word) and the compacted list, kept across the passes of a frame
static int adaptive_bind(hjr_ctx* c, const ParamsW* p, const FrameGeom& g, KParams& kp)
{
    hjr_ctx::Adaptive& ad = c->ad;
    if (!ad.state.reserve(((size_t)g.owned + 1u) * 4u) || !ad.list.reserve((size_t)g.owned * 4u)) {
        set_error("hjr_render: adaptive-sampling buffer allocation failed");
        return HJR_ERR_DEVICE;
    }
    kp.ad_state = (uint32_t*)ad.state.p;
    kp.ad_threshold = ad.threshold;
    const uint32_t gr = g.chunk_spp, ms = ad.min_samples ? (ad.min_samples + gr - 1) / gr * gr : 2u * gr;
    kp.ad_decide = (g.pr.end < p->spp && g.pr.end >= ms && g.pr.end / gr >= 2u) ? 1u : 0u;
    return HJR_OK;
}
// ... after order_tiles: the stopped tiles leave the launch's tile list (stable: the cost order survives)
static int adaptive_filter(hjr_ctx* c, KParams& kp, hipStream_t st)
{
    kp.ad_src = kp.tile_order; kp.ad_list = (uint32_t*)c->ad.list.p;
    hipLaunchKernelGGL(hjr_filter_tiles_kernel, dim3(1), dim3(1024), 0, st, kp);
    HIPCHK(hipGetLastError());
    kp.tile_order = kp.ad_list;
    return HJR_OK;
}
// the count of tiles still active goes to the host, behind the kernel that took the pass's stop decisions
static int adaptive_count(hjr_ctx* c, const FrameGeom& g, hipStream_t st)
{
    HIPCHK(hipMemcpyAsync(c->ad.h_active, (uint32_t*)c->ad.state.p + g.owned, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(c->ad.ready, st));
    return HJR_OK;
}
// ... after the render kernel, for every launch: sums of the sample chunks -> pixel means (a sample pass: -> running sums and running means;
// an adaptive one: statistic and stop decisions too, then the count of tiles still active goes to the host).  d_var: the variance AOV was
// requested (hjr_render_var); a frame of a single chunk has no chunk sums and gets the fill.
// count_later: hjr_firefly_kernel decides behind this kernel (rule 10) and the caller sends the count after it
static int finalize_chunks(hjr_ctx* c, const FrameGeom& g, KParams& kp, bool adaptive, bool count_later, float* d_var, hipStream_t st)
{
    using Kernel = void (*)(KParams, float*);
    static const Kernel kernels[2][2][2] = { // [pass][adaptive][variance]
        { { hjr_finalize_kernel<false, false, false>, hjr_finalize_kernel<false, false, true> }, { nullptr, nullptr } },
        { { hjr_finalize_kernel<true, false, false>, hjr_finalize_kernel<true, false, true> }, { hjr_finalize_kernel<true, true, false>, hjr_finalize_kernel<true, true, true> } },
    };
    const size_t n_slots = (size_t)g.owned * 64u;
    if (n_slots == 0) return HJR_OK;
    Kernel kern = g.n_chunks > 1 ? kernels[g.pr.pass][adaptive][d_var != nullptr] : d_var ? hjr_fill_var_kernel : nullptr;
    if (!kern) return HJR_OK;
    if (g.pr.pass && (adaptive || d_var)) { // the statistic, kept across the passes of a frame
        if (!c->d_stat.reserve(n_slots * sizeof(float2))) { set_error("hjr_render: statistic buffer allocation failed"); return HJR_ERR_DEVICE; }
        kp.stat = (float2*)c->d_stat.p;
    }
    uint32_t* const d_count = adaptive ? (uint32_t*)c->ad.state.p + g.owned : nullptr;
    if (adaptive) HIPCHK(hipMemsetAsync(d_count, 0, 4, st));
    const unsigned fb = (unsigned)std::max<size_t>(1, std::min<size_t>((n_slots + 255) / 256, (size_t)c->n_cus * 8));
    hipLaunchKernelGGL(kern, dim3(fb), dim3(256), 0, st, kp, d_var);
    HIPCHK(hipGetLastError());
    if (adaptive && !count_later) return adaptive_count(c, g, st);
    return HJR_OK;
}

// the launch of both rules: hjr_firefly_kernel over the owned pixels' first m (<= 64, hjr_layout.h) colour chunk sums, in the instantiation
// of a one-shot frame, a sample pass or an adaptive sample pass
static int firefly_launch(hjr_ctx* c, const FrameGeom& g, const KParams& kp, uint32_t m, bool pass, bool adaptive, hipStream_t st)
{
    constexpr uint32_t FB = 128; // lanes per workgroup: 64 chunks x 128 lanes x 4 bytes = 32 KiB of LDS at most
    using Kernel = void (*)(const KParams, const float, unsigned long long*);
    // (instantiated in the order they always were: it is their order in the code object)
    static const Kernel kernels[3] = { hjr_firefly_kernel<FB, false, false>, hjr_firefly_kernel<FB, true, true>, hjr_firefly_kernel<FB, true, false> };
    const size_t n_slots = (size_t)g.owned * 64u;
    const unsigned fb = (unsigned)std::max<size_t>(1, std::min<size_t>((n_slots + FB - 1) / FB, (size_t)c->n_cus * 16));
    hipLaunchKernelGGL(kernels[pass ? (adaptive ? 1 : 2) : 0], dim3(fb), dim3(FB), (size_t)m * FB * sizeof(float), st, kp, (float)c->opt.get(hjr::OPT_FIREFLY_CLAMP, 0),
                       (unsigned long long*)((char*)c->d_work.p + WorkArea::FIREFLY));
    return launched();
}
// Option "firefly_clamp" (hjr_firefly_kernel, DESIGN.md §4 rule 9), behind finalize_chunks on a one-shot frame: the colour of the pixels with a
// chunk over their limit is rewritten.  With the option off, or a frame of fewer than 4 full chunks, nothing is launched.
static int firefly_clamp(hjr_ctx* c, const ParamsW* p, const FrameGeom& g, const KParams& kp, hipStream_t st)
{
    const uint32_t m = p->spp / g.chunk_spp;
    if (c->opt.get(hjr::OPT_FIREFLY_CLAMP, 0) <= 0 || g.pr.pass || g.n_chunks < 2 || m < 4 || g.owned == 0) return HJR_OK;
    return firefly_launch(c, g, kp, m, false, false, st);
}
// Option "firefly_clamp_passes" (DESIGN.md §4 rule 10), behind finalize_chunks on a sample pass of a frame that keeps its colour chunk sums
// (firefly_keeps_chunks) and has received m_n = sample_end / granule >= 4 full chunks: the colour of the pixels with a chunk over their limit
// is rewritten from chunks [0, m_n) (a stopped tile of an adaptive frame: from its own), and with `decide` the kernel takes the adaptive
// pass's stop decisions from the clamped sums (finalize_chunks ran with ad_decide 0).  Earlier passes launch nothing: the parent's sequence.
static bool firefly_pass_acts(const hjr_ctx* c, const FrameGeom& g)
{
    return g.pr.pass && g.n_chunks > 1 && g.owned > 0 && hjr::firefly_keeps_chunks(c) && g.pr.end / g.chunk_spp >= 4u;
}
static int firefly_clamp_pass(hjr_ctx* c, const FrameGeom& g, const KParams& kp, bool adaptive, bool decide, hipStream_t st)
{
    if (!firefly_pass_acts(c, g)) return HJR_OK;
    KParams kf = kp;
    kf.ad_decide = decide ? 1u : 0u;
    return firefly_launch(c, g, kf, g.pr.end / g.chunk_spp, true, adaptive, st);
}

// Option "adaptive_temporal" (DESIGN.md §4 rule 11), behind finalize_chunks on a deciding pass of an adaptive frame with a prior: one wave per
// owned tile, the finalize dispatch's shape.  finalize_chunks ran with ad_decide 0 and left the statistic in kp.stat.
static int adaptive_temporal_launch(hjr_ctx* c, const FrameGeom& g, const KParams& kp, const void* d_prior, hipStream_t st)
{
    const size_t n_slots = (size_t)g.owned * 64u;
    const unsigned fb = (unsigned)std::max<size_t>(1, std::min<size_t>((n_slots + 255) / 256, (size_t)c->n_cus * 8));
    hipLaunchKernelGGL(hjr_adaptive_temporal_kernel, dim3(fb), dim3(256), 0, st, kp, (const float4*)d_prior);
    return launched();
}

// pr: check_pass of this call, made before the caller enqueued anything
// d_var: the variance AOV (one float per pixel) or null
// d_prior: option "adaptive_temporal" in effect and the frame has a prior (hjr_render_denoised): rule 11 takes an adaptive pass's decisions
int hjr::render_impl(hjr_ctx* c, const ParamsW* p, const PassRange& pr, void* d_color, void* d_albedo, void* d_normal, void* d_var, hipStream_t st, const void* d_prior)
{
    FrameGeom g;
    KParams kp;
    int rc;
    if ((rc = hjr::frame_geometry(c, p, d_color, pr, g)) != HJR_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    // adaptive sampling acts on sample passes only; with it off (or a whole-frame render) nothing below differs from the plain launch
    const bool adaptive = pr.pass && c->ad.threshold > 0.0f && g.owned > 0;
    uint32_t active = (uint32_t)g.owned;
    if (adaptive && (rc = adaptive_items(c, g, active)) != HJR_OK) return rc;
    if ((rc = bind_params(c, p, g, d_color, d_albedo, d_normal, d_var, st, kp)) != HJR_OK) return rc;
    if (adaptive && (rc = adaptive_bind(c, p, g, kp)) != HJR_OK) return rc;
    HIPCHK(hipEventRecord(c->ev0, st));
    if (!adaptive || active > 0) { // (an adaptive pass with no active tile launches no render kernel and still writes the AOVs)
        if ((rc = order_tiles(c, p, g, kp, st)) != HJR_OK) return rc;
        if (adaptive && active < g.owned && (rc = adaptive_filter(c, kp, st)) != HJR_OK) return rc;
        if ((rc = launch_render(c, p, g, kp, st)) != HJR_OK) return rc;
    }
    // rule 10: on a deciding pass of >= 4 full chunks the decision is hjr_firefly_kernel's, from the clamped sums
    const bool decide = adaptive && kp.ad_decide != 0u, ff_decides = decide && firefly_pass_acts(c, g);
    // rule 11: with a prior the decision is hjr_adaptive_temporal_kernel's (the caller refused the pair with rule 10)
    const bool at_decides = decide && !ff_decides && d_prior != nullptr;
    if (ff_decides || at_decides) kp.ad_decide = 0u;
    if ((rc = finalize_chunks(c, g, kp, adaptive, ff_decides || at_decides, (float*)d_var, st)) != HJR_OK) return rc;
    if ((rc = firefly_clamp(c, p, g, kp, st)) != HJR_OK) return rc;
    if ((rc = firefly_clamp_pass(c, g, kp, adaptive, ff_decides, st)) != HJR_OK) return rc;
    if (at_decides && (rc = adaptive_temporal_launch(c, g, kp, d_prior, st)) != HJR_OK) return rc;
    if ((ff_decides || at_decides) && (rc = adaptive_count(c, g, st)) != HJR_OK) return rc;
    HIPCHK(hipEventRecord(c->ev1, st));
    c->event_pending = true;
    if (pr.pass && c->opt.get(hjr::OPT_VERBOSE, 0))
        fprintf(stderr, "[hjr] frame %u: sample pass [%u, %u) of %u spp, chunks %u..%u of %u\n", p->frame, pr.begin, pr.end, p->spp, g.chunk0, g.chunk0 + g.pass_chunks - 1, g.n_chunks);
    hjr_ctx::Adaptive& ad = c->ad;
    ad.frame = adaptive;
    if (adaptive) {
        ad.owned = (uint32_t)g.owned; ad.last_end = pr.end;
        ad.samples = (pr.begin ? ad.samples : 0ull) + (uint64_t)active * (pr.end - pr.begin) * 64ull;
        if (c->opt.get(hjr::OPT_VERBOSE, 0))
            fprintf(stderr, "[hjr] frame %u: adaptive pass [%u, %u): %u of %u tiles active, %llu samples rendered so far%s\n", p->frame, pr.begin, pr.end, active, ad.owned,
                    (unsigned long long)ad.samples, decide ? ", stop decision after it" : "");
    }
    end_pass(c, p, pr);
    return HJR_OK;
}

extern "C" int hjr_set_adaptive(hjr_ctx* c, const hjr_adaptive* a_user)
{
    if (!c) { set_error("hjr_set_adaptive: null context"); return HJR_ERR_ARG; }
    hjr_adaptive a; // sized struct
    memset(&a, 0, sizeof(a));
    if (a_user && !hjr::abi_take(a_user, a, "hjr_set_adaptive")) return HJR_ERR_ARG;
    if (!std::isfinite(a.noise_threshold) || a.noise_threshold < 0.0f) { set_error("hjr_set_adaptive: noise_threshold must be finite and >= 0"); return HJR_ERR_ARG; }
    if (a.min_samples > 0x7fffffffu) { set_error("hjr_set_adaptive: min_samples out of range"); return HJR_ERR_ARG; }
    c->ad.threshold = a.noise_threshold; c->ad.min_samples = a.min_samples;
    c->ad.frame = false;
    c->pass.active = false; // an unfinished progressive frame ends: it cannot change its rule half way
    return HJR_OK;
}

extern "C" int hjr_get_adaptive_state(hjr_ctx* c, hjr_adaptive_state* out)
{
    if (!c || !out) { set_error("hjr_get_adaptive_state: null argument"); return HJR_ERR_ARG; }
    uint32_t out_size;
    if (!hjr::abi_size(out, out_size, "hjr_get_adaptive_state")) return HJR_ERR_ARG;
    if (!c->ad.frame) { set_error("hjr_get_adaptive_state: the context's last render was not an adaptive sample pass"); return HJR_ERR_STATE; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ad.ready));
    hjr_adaptive_state s;
    memset(&s, 0, sizeof(s));
    s.struct_size = (uint32_t)sizeof(s);
    s.owned_tiles = c->ad.owned; s.active_tiles = *c->ad.h_active; s.sample_end = c->ad.last_end; s.samples_rendered = c->ad.samples;
    return hjr::abi_give(out, s, "hjr_get_adaptive_state") ? HJR_OK : HJR_ERR_ARG;
}

extern "C" int hjr_copy_tile_samples(hjr_ctx* c, uint32_t* dst, size_t n_owned_tiles)
{
    if (!c || !dst) { set_error("hjr_copy_tile_samples: null argument"); return HJR_ERR_ARG; }
    if (!c->ad.frame) { set_error("hjr_copy_tile_samples: the context's last render was not an adaptive sample pass"); return HJR_ERR_STATE; }
    if (n_owned_tiles != c->ad.owned) { set_error("hjr_copy_tile_samples: n_owned_tiles must be hjr_adaptive_state.owned_tiles = " + std::to_string(c->ad.owned)); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ad.ready));
    HIPCHK(hipMemcpy(dst, c->ad.state.p, n_owned_tiles * 4u, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n_owned_tiles; i++)
        if (dst[i] == 0u) dst[i] = c->ad.last_end; // still active: it has received every sample so far
    return HJR_OK;
}

extern "C" int hjr_render_device_var(hjr_ctx* c, const hjr_params* p_user, void* d_color, void* d_albedo, void* d_normal, void* d_variance, void* stream)
{
    ParamsW params; // sized struct (the long form: the render window behind hjr_params)
    if (!take_params(c, p_user, params, "hjr_render_device")) return HJR_ERR_ARG;
    const ParamsW* p = &params;
    WorkRect rect; // (a bad window is HJR_ERR_ARG ahead of the pass rules, as in hjr_render_var)
    if (const int rc = work_rect(p, "hjr_render", rect)) return rc;
    PassRange pr;
    if (const int rc = hjr::check_pass(c, p, (d_color ? 1u : 0u) | (d_albedo ? 2u : 0u) | (d_normal ? 4u : 0u) | (d_variance ? 8u : 0u), pr)) return rc;
    return hjr::render_impl(c, p, pr, d_color, d_albedo, d_normal, d_variance, stream_of(c, stream));
}
extern "C" int hjr_render_device(hjr_ctx* c, const hjr_params* p_user, void* d_color, void* d_albedo, void* d_normal, void* stream)
{
    return hjr_render_device_var(c, p_user, d_color, d_albedo, d_normal, nullptr, stream);
}

extern "C" int hjr_render_var(hjr_ctx* c, const hjr_params* p_user, float* color, float* albedo, float* normal, float* variance)
{
    if (!c || !p_user || !color) { set_error("hjr_render: null argument"); return HJR_ERR_ARG; }
    ParamsW params; // sized struct (the long form: the render window behind hjr_params)
    if (!take_params(c, p_user, params, "hjr_render")) return HJR_ERR_ARG;
    const ParamsW* p = &params;
    HIPCHK(hipSetDevice(c->device));
    if ((size_t)p->width * p->height == 0) { set_error("hjr_render: empty image"); return HJR_ERR_ARG; }
    // HJR_FLAG_PACKED: the buffers hold this rank's tiles only (hjr_owned_tiles x 64 float4), as in hjr_render_device
    const bool packed_out = (p->flags & HJR_FLAG_PACKED) != 0;
    if (p->rank >= (p->world_size ? p->world_size : 1u)) { set_error("hjr_render: rank >= world_size"); return HJR_ERR_ARG; }
    WorkRect rect; // the host buffers are the work rectangle's size: the window's, or else the frame's
    if (const int rc = work_rect(p, "hjr_render", rect)) return rc;
    const size_t bytes = packed_out ? (size_t)hjr_owned_tiles(rect.w, rect.h, p->rank, p->world_size ? p->world_size : 1u) * 64u * 16u : (size_t)rect.w * rect.h * 16;
    PassRange pr;
    if (const int rc = hjr::check_pass(c, p, 1u | (albedo ? 2u : 0u) | (normal ? 4u : 0u) | (variance ? 8u : 0u), pr)) return rc;
    if (bytes == 0) { end_pass(c, p, pr); return HJR_OK; } // a rank without tiles
    DevBuf* bufs[4] = { &c->d_color, &c->d_albedo, &c->d_normal, &c->d_variance };
    float* host[4] = { color, albedo, normal, variance };
    const size_t len[4] = { bytes, bytes, bytes, bytes / 4 }; // (the variance is one float per pixel: a quarter of an AOV's bytes)
    for (int i = 0; i < 4; i++) {
        if (!host[i]) continue;
        if (!bufs[i]->reserve(len[i])) { set_error("hjr_render: AOV allocation failed"); return HJR_ERR_DEVICE; }
        if (!packed_out) HIPCHK(hipMemsetAsync(bufs[i]->p, 0, len[i], c->stream));
    }
    HostStage hs(c);
    hs.rc = hjr::render_impl(c, p, pr, c->d_color.p, albedo ? c->d_albedo.p : nullptr, normal ? c->d_normal.p : nullptr, variance ? c->d_variance.p : nullptr, c->stream);
    for (int i = 0; i < 4; i++)
        if (host[i]) hs.down(host[i], bufs[i]->p, len[i]);
    return hs.finish("hjr_render"); // drains the stream: CUDA_SYNC_CHECK (renderer.h:1242)
}
extern "C" int hjr_render(hjr_ctx* c, const hjr_params* p_user, float* color, float* albedo, float* normal)
{
    return hjr_render_var(c, p_user, color, albedo, normal, nullptr);
}
