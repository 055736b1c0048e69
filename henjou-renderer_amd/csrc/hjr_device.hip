// Device context of libhenjou_hip.so: HBM-resident scene, per-frame BVH upload, kernel launch and timing.
// Replaces the reference's CUDA/OptiX plumbing (renderer/renderer.h:197-255 upload, 293-739 context/GAS/IAS/pipeline/SBT,
// 1175-1242 Params fill + optixLaunch).  No CPU fallback exists: without a gfx950 device every entry point fails loudly.
#include <hip/hip_runtime.h>
#include <chrono>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/henjou_hip.h"
#include "../host/frame.hpp"
#include "hjr_launch.hip.h"
#if defined(HJR_UNITY) && !defined(HJR_LEAN_VARIANT)
#define HJR_TRACE_UNIT /* one translation unit: the hook's kernels and their launch code are compiled here (hjr_launch_trace.hip is included below) */
#endif
#include "hjr_trace_hook.hip.h"
#include "../host/abi.hpp"
#include "hjr_aux.hip.h"
#include "hjr_denoise.hip.h"
#include "hjr_temporal.hip.h"

#define HIPCHK(call)                                                                                            \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess) {                                                                                 \
            set_error(std::string(#call) + " failed: " + hipGetErrorString(e_));                               \
            return HJR_ERR_DEVICE;                                                                              \
        }                                                                                                       \
    } while (0)

// behind the last launch of a function: the runtime's verdict on what was enqueued
static int launched() { HIPCHK(hipGetLastError()); return HJR_OK; }
// the stream an entry point enqueues on: the caller's, or the context's own
static hipStream_t stream_of(const hjr_ctx* c, void* hip_stream) { return hip_stream ? (hipStream_t)hip_stream : c->stream; }
// grid of the image kernels: 256 threads take 64 x 4 pixels
static dim3 image_grid(uint32_t w, uint32_t h) { return dim3((w + 63) / 64, (h + 3) / 4); }
// the sized hjr_params of entry point `who`, whose name the refusals carry; false: HJR_ERR_ARG
static bool take_params(const hjr_ctx* c, const hjr_params* p_user, ParamsW& p, const char* who)
{
    if (!c) { set_error(std::string(who) + ": null context"); return false; }
    // (abi_take for a caller's hjr_params or hjr_params_window: the window is read iff the caller's struct_size covers it, else it is 0)
    uint32_t n;
    if (!hjr::abi_size(p_user, n, who)) return false;
    memset(static_cast<void*>(&p), 0, sizeof(p));
    memcpy(static_cast<void*>(&p), p_user, std::min<size_t>(n, sizeof(p)));
    p.struct_size = (uint32_t)sizeof(p);
    return true;
}
// LaunchPlan::lds_mode of frame data: the builder's 0 BVH4 in memory, 1 / 2 BVH2 staged in LDS, and 3 for a BVH2 it left in memory
static int launch_layout(const hjr::FrameData& f) { return f.lds_mode == 0 && f.width == 2 ? 3 : f.lds_mode; }

// The work rectangle of a render call: the window (hjr_params_window.window, include/henjou_hip.h), or else the frame.  The one place that reads the
// window: the tile grid, the owned tiles, the items and every buffer size follow from w x h; x0, y0 reach the kernels as the origin of the
// full-frame coordinates (KParams::win_word).  p->width and p->height are positive (the callers check).
struct WorkRect {
    uint32_t x0 = 0, y0 = 0, w = 0, h = 0;
    bool window = false;
    uint64_t key() const { return window ? ((uint64_t)x0 << 39) ^ ((uint64_t)y0 << 26) ^ ((uint64_t)w << 13) ^ (uint64_t)h ^ (1ull << 52) : 0ull; } // 0 = no window; one-to-one below 8192
};
static bool has_window(const ParamsW* p) { return p->window[2] != 0u; }
static int work_rect(const ParamsW* p, const char* who, WorkRect& r)
{
    r = WorkRect();
    r.w = p->width; r.h = p->height;
    if (!has_window(p)) return HJR_OK;
    const uint32_t x0 = p->window[0], y0 = p->window[1], x1 = p->window[2], y1 = p->window[3];
    const std::string text = std::string(who) + ": window [" + std::to_string(x0) + ", " + std::to_string(x1) + ") x [" + std::to_string(y0) + ", " + std::to_string(y1) + ") of a " +
                             std::to_string(p->width) + " x " + std::to_string(p->height) + " frame: ";
    if (x0 >= x1 || y0 >= y1) { set_error(text + "window needs x0 < x1 and y0 < y1"); return HJR_ERR_ARG; }
    if (x1 > p->width || y1 > p->height) { set_error(text + "window needs x1 <= width and y1 <= height"); return HJR_ERR_ARG; }
    if (x0 % HJR_TILE || y0 % HJR_TILE) { set_error(text + "window needs x0 and y0 to be multiples of " + std::to_string(HJR_TILE)); return HJR_ERR_ARG; }
    r.x0 = x0; r.y0 = y0; r.w = x1 - x0; r.h = y1 - y0; r.window = true;
    return HJR_OK;
}
// the entry points whose filters need neighbours outside a window take whole frames only
static int refuse_window(const ParamsW* p, const char* who)
{
    if (!has_window(p)) return HJR_OK;
    set_error(std::string(who) + ": a render window (hjr_params_window.window) is not supported here (the filters and the G-buffer pass need the pixels around a window); render the whole frame");
    return HJR_ERR_ARG;
}

// Host buffers through device buffers on the context's stream: every entry point that takes host image pointers.  Uploads, the caller's
// launch (into `rc`) and downloads each happen only while everything before them succeeded; finish() drains the stream on every path, so no
// such entry point returns while a copy it enqueued is in flight, and folds the first error.  `buf` is the temporary buffer of the entry
// points that stage through no context-owned one (empty for the others), released only after the stream has drained.
struct HostStage {
    hjr_ctx* c;
    DevBuf buf;
    int rc = HJR_OK;           // of the launch
    hipError_t e = hipSuccess; // the first failed runtime call
    explicit HostStage(hjr_ctx* c_) : c(c_) {}
    bool ok() const { return rc == HJR_OK && e == hipSuccess; }
    void up(void* dst, const void* src, size_t n) { if (ok() && n) e = hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, c->stream); }
    void down(void* dst, const void* src, size_t n) { if (ok() && n) e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->stream); }
    int finish(const char* who)
    {
        const hipError_t es = hipStreamSynchronize(c->stream);
        buf.release(); // explicitly, behind the drain
        if (rc != HJR_OK) return rc;
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) { set_error(std::string(who) + ": " + hipGetErrorString(e)); return HJR_ERR_DEVICE; }
        return HJR_OK;
    }
};

extern "C" int hjr_create(int device, hjr_ctx** out)
{
    if (!out) { set_error("hjr_create: null out pointer"); return HJR_ERR_ARG; }
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error(std::string("hjr_create: no HIP device available (") + hipGetErrorString(e) + "); this library has no CPU fallback");
        return HJR_ERR_DEVICE;
    }
    if (device < 0 || device >= n) { set_error("hjr_create: device ordinal out of range"); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(std::string("hjr_create: device is ") + prop.gcnArchName + ", this library carries gfx950 (MI355X) code objects only");
        return HJR_ERR_DEVICE;
    }
    hjr_ctx* c = new hjr_ctx();
    c->device = device;
    c->n_cus = prop.multiProcessorCount;
    memset(&c->stats, 0, sizeof(c->stats));
#ifdef HJR_ENV_OPTIONS /* experiment builds only (make variant): every option also from the environment, HJR_<KEY> */
    for (int i = 0; i < hjr::OPT_COUNT; i++) {
        std::string name = std::string("HJR_") + hjr::opt_table()[i].key;
        for (char& ch : name) ch = (char)toupper((unsigned char)ch);
        if (const char* e = getenv(name.c_str())) { const int v = atoi(e); if (v >= hjr::opt_table()[i].lo && v <= hjr::opt_table()[i].hi) c->opt.v[i] = v; }
    }
    if (c->opt.is_set(hjr::OPT_HOST_THREADS)) hjr::set_host_threads(c->opt.v[hjr::OPT_HOST_THREADS]);
#endif
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess ||
        hipEventCreate(&c->ev1) != hipSuccess) {
        set_error("hjr_create: stream/event creation failed");
        delete c;
        return HJR_ERR_DEVICE;
    }
    *out = c;
    return HJR_OK;
}

// Tuning / test options (host/options.hpp lists keys, ranges and defaults; include/henjou_hip.h documents them)
extern "C" int hjr_set_option(hjr_ctx* c, const char* key, int value)
{
    if (!c) { set_error("hjr_set_option: null context"); return HJR_ERR_ARG; }
    const int i = hjr::opt_find(key);
    if (i < 0) { set_error(std::string("hjr_set_option: unknown option \"") + (key ? key : "(null)") + "\""); return HJR_ERR_ARG; }
    const hjr::OptDesc& d = hjr::opt_table()[i];
    if (value != -1 && (value < d.lo || value > d.hi || hjr::opt_hole(i, value))) {
        set_error(std::string("hjr_set_option: value out of range for \"") + d.key + "\" (" + std::to_string(d.lo) + " .. " + std::to_string(d.hi) + ", or -1 for the default)");
        return HJR_ERR_ARG;
    }
    c->opt.v[i] = value;
    // rule 10 keeps chunk sums from a frame's first pass on: an unfinished progressive frame cannot change its rule half way (as hjr_set_adaptive).
    // "firefly_clamp" alone with "firefly_clamp_passes" off keeps what it always did: the next pass is refused by check_pass
    if (i == hjr::OPT_FIREFLY_CLAMP_PASSES || (i == hjr::OPT_FIREFLY_CLAMP && c->opt.get(hjr::OPT_FIREFLY_CLAMP_PASSES, 0) == 1)) { c->pass.active = false; c->ad.frame = false; }
    if (i == hjr::OPT_ADAPTIVE_TEMPORAL) { c->pass.active = false; c->ad.frame = false; c->tmp.have_prior = false; } // rule 11: an unfinished progressive frame cannot change its rule half way (as hjr_set_adaptive); the history stays
    if (i == hjr::OPT_DENOISE_TEMPORAL || i == hjr::OPT_DENOISE_VARIANCE_SPATIAL || i == hjr::OPT_DENOISE_TEMPORAL_COVERAGE || i == hjr::OPT_DENOISE_TEMPORAL_MOMENTS || i == hjr::OPT_DENOISE_TEMPORAL_RESPONSE) c->tmp.have_prev = false; // setting any of these options drops the history
    if (i == hjr::OPT_HOST_THREADS) hjr::set_host_threads(value);
    return HJR_OK;
}
extern "C" int hjr_get_option(hjr_ctx* c, const char* key, int* value)
{
    if (!c || !value) { set_error("hjr_get_option: null argument"); return HJR_ERR_ARG; }
    const int i = hjr::opt_find(key);
    if (i < 0) { set_error(std::string("hjr_get_option: unknown option \"") + (key ? key : "(null)") + "\""); return HJR_ERR_ARG; }
    *value = c->opt.v[i];
    return HJR_OK;
}

extern "C" void hjr_destroy(hjr_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    if (c->ad.h_active) (void)hipHostFree(c->ad.h_active);
    if (c->ad.ready) (void)hipEventDestroy(c->ad.ready);
    c->dbvh.release();
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c; // every DevBuf of the context, with its device still current
}

extern "C" int hjr_upload_scene(hjr_ctx* c, const hjr_scene_view* v)
{
    if (!c || !v) { set_error("hjr_upload_scene: null argument"); return HJR_ERR_ARG; }
    hjr_scene_view view; // sized struct: only the bytes the caller owns are read
    if (!hjr::abi_take(v, view, "hjr_upload_scene")) return HJR_ERR_ARG;
    v = &view;
    std::string err;
    if (!c->scene.set(*v, err)) { set_error("hjr_upload_scene: " + err); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    static_assert(sizeof(hjr_material) == HJR_MAT_F4 * 16, "hjr_material must be HJR_MAT_F4 x float4");
    if (!c->d_materials.upload(c->scene.materials.data(), c->scene.materials.size() * sizeof(hjr_material), c->stream)) {
        set_error("hjr_upload_scene: material upload failed");
        return HJR_ERR_DEVICE;
    }
    // textureBind (renderer.h:740-800): RGBA8 atlas + per-slot descriptors + the sRGB decode table
    c->n_textures = (uint32_t)c->scene.textures.size();
    if (c->n_textures) {
        std::vector<uint32_t> desc;
        for (auto& t : c->scene.textures) { desc.push_back(t.offset); desc.push_back(t.width); desc.push_back(t.height); desc.push_back((uint32_t)t.srgb); }
        float lut[256];
        for (int i = 0; i < 256; i++) {
            double v = (double)i / 255.0;
            lut[i] = (float)(v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4));
        }
        if (!c->d_texels.upload(c->scene.texels.data(), c->scene.texels.size() * 4, c->stream) ||
            !c->d_tex_desc.upload(desc.data(), desc.size() * 4, c->stream) || !c->d_srgb_lut.upload(lut, sizeof(lut), c->stream)) {
            set_error("hjr_upload_scene: texture upload failed");
            return HJR_ERR_DEVICE;
        }
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->frame_gen++;
    c->tmp.have_prev = false; // temporal history: another scene
    c->have_scene = true;
    c->have_frame = false;
    c->dbvh.have_scene = false; // the device builder uploads the new scene at its next build
    c->dbvh.topo.valid = false; // ... and "device_bvh_instances" builds its topology again
    c->refit = hjr_ctx::Refit(); // ... which is a full one
    return HJR_OK;
}

// updateIASMatrix + buildIAS (renderer.h:257-291, 398-490) in two halves, so that a frame loop can prepare frame f + 1 on the
// host (worker threads, no device access, no access to what a running render reads) while frame f renders:
//   hjr_prepare_transforms: flatten + BVH build into the context's prepared frame (hjr_ctx::prep);
//   hjr_commit_transforms:  upload the prepared data (after the previous render has finished) and make it current (hjr_ctx::built).
// hjr_set_transforms = prepare + commit.
extern "C" int hjr_prepare_transforms(hjr_ctx* c, const float* m, const float* inv, uint32_t n)
{
    if (!c || (n && (!m || !inv))) { set_error("hjr_set_transforms: null argument"); return HJR_ERR_ARG; }
    if (!c->have_scene) { set_error("hjr_set_transforms: no scene uploaded"); return HJR_ERR_STATE; }
    std::string err;
    hjr::BuildOptions bo; // options "lds_bvh", "lds_stack16", "bvh_width", "leaf_max", "verbose" (host build stages)
    bo.allow_lds = c->opt.get(hjr::OPT_LDS_BVH, 1) != 0;
    bo.prefer_stack16 = c->opt.get(hjr::OPT_LDS_STACK16, 0) != 0;
    bo.bvh_width = c->opt.get(hjr::OPT_BVH_WIDTH, -1);
    bo.leaf_max = c->opt.get(hjr::OPT_LEAF_MAX, -1);
    bo.refine = c->opt.get(hjr::OPT_BVH_REFINE, -1);
    bo.timing = c->opt.get(hjr::OPT_VERBOSE, 0) != 0;
    const bool device = c->opt.get(hjr::OPT_DEVICE_BVH, 0) != 0; // option "device_bvh": the build runs at hjr_commit_transforms
    if (device && (bo.bvh_width == 2 || c->opt.get(hjr::OPT_LDS_BVH, -1) == 1)) {
        set_error("hjr_set_transforms: \"device_bvh\" builds the BVH4 memory layout only; it cannot be combined with \"bvh_width\" 2 or \"lds_bvh\" 1");
        return HJR_ERR_ARG;
    }
    BuildKey key;
    key.allow_lds = bo.allow_lds; key.prefer_stack16 = bo.prefer_stack16; key.bvh_width = bo.bvh_width; key.leaf_max = bo.leaf_max; key.refine = bo.refine;
    key.device = device;
    key.opt_rounds = device ? (uint32_t)c->opt.get(hjr::OPT_DEVICE_BVH_OPT, 0) : 0u;
    key.instances = device && c->opt.get(hjr::OPT_DEVICE_BVH_INSTANCES, 0) != 0;
    key.graft = key.instances && c->opt.get(hjr::OPT_DEVICE_BVH_GRAFT, 0) != 0;
    hjr_ctx::Prepared& pp = c->prep;
    pp.valid = false;
    pp.same = false;
    // unchanged instance transforms (static geometry, e.g. a camera-only animation): the world-space arrays and the BVH of the
    // previous frame are still right; the reference re-uploads its IAS every frame (renderer.h:257-291), which costs it nothing
    const bool force_rebuild = c->opt.get(hjr::OPT_FORCE_REBUILD, 0) != 0; // benchmarking option
    if (!force_rebuild && c->have_frame && c->built.key == key && c->built.m.size() == (size_t)n * 12 && n == c->scene.n_instances &&
        (n == 0 || (memcmp(c->built.m.data(), m, (size_t)n * 48) == 0 && memcmp(c->built.inv.data(), inv, (size_t)n * 48) == 0))) {
        pp.same = true;
        pp.valid = true;
        return HJR_OK;
    }
    const auto t_build0 = std::chrono::steady_clock::now();
    if (device) { // validation and the light table here; flatten + BVH at the commit, on the device
        if (n != c->scene.n_instances) { set_error("hjr_set_transforms: instance count does not match the uploaded scene"); return HJR_ERR_ARG; }
        pp.frame = hjr::FrameData();
        pp.frame.n_tris = c->scene.n_triangles;
        pp.frame.width = 4;
        pp.frame.lds_mode = 0;
        hjr::build_lights(c->scene, m, inv, pp.frame);
    } else if (!hjr::build_frame(c->scene, m, inv, n, bo, pp.frame, err)) { set_error("hjr_set_transforms: " + err); return HJR_ERR_ARG; }
    pp.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build0).count();
    pp.m.assign(m, m + (size_t)n * 12); pp.inv.assign(inv, inv + (size_t)n * 12); pp.key = key;
    pp.valid = true;
    return HJR_OK;
}

// option "device_bvh": the build of the prepared transforms as kernels on the context's stream, behind what is already queued there.
// It writes the builder's own buffers; they become current (swapped with d_nodes, d_tri_*, d_lights) only when it succeeds, so a
// failed build leaves the previous frame current.
// Option "device_bvh_refit": up to that many consecutive commits after a full build keep its topology and refit the boxes
// (hjr::device_bvh_refit), while the current data is a device build of this scene with these build options and the cost guard holds.
// `instances`: the instance subtrees the build made (0: an ordinary build or a refit), for hjr_stats and the verbose line.
static int commit_device(hjr_ctx* c, uint32_t& instances)
{
    const int leaf_max = c->opt.get(hjr::OPT_LEAF_MAX, (int)HJR_LEAF_DEFAULT);
    const int opt_rounds = c->opt.get(hjr::OPT_DEVICE_BVH_OPT, 0); // option "device_bvh_opt": treelet-restructuring rounds
    const uint32_t limit = (uint32_t)c->opt.get(hjr::OPT_DEVICE_BVH_REFIT, 0);
    hjr_ctx::Prepared& pp = c->prep;
    const uint32_t n_inst = (uint32_t)(pp.m.size() / 12), tag = pp.key.pack();
    hjr_ctx::Refit& rf = c->refit;
    // key.instances: per-instance trees kept in dbvh.topo, a top tree per commit; no refits with it
    // key.graft (only ever set with it): the instances' BVH4s collapsed once, grafted under a BVH4 top tree
    if (!pp.key.instances) c->dbvh.drop_topology();
    const bool refit = !pp.key.instances && c->have_frame && rf.device && c->dbvh.have_scene && !rf.rebuild && rf.count < limit && rf.tag == tag &&
                       c->built.m.size() == pp.m.size() && c->scene.n_triangles >= 2 && c->frame.n_tris == c->scene.n_triangles;
    hjr::DeviceBvhResult r;
    std::string err;
    hjr::FrameData& f = pp.frame;
    const int rc = pp.key.instances ? hjr::device_bvh_instances(c->dbvh, c->scene, pp.m.data(), pp.inv.data(), n_inst, (uint32_t)leaf_max, (uint32_t)opt_rounds, tag, pp.key.graft,
                                                                f.lights.data(), f.lights.size(), c->stream, r, err)
                   : refit ? hjr::device_bvh_refit(c->dbvh, c->scene, pp.m.data(), pp.inv.data(), n_inst, c->d_nodes, c->d_tri_geom, c->frame.n_nodes,
                                                 f.lights.data(), f.lights.size(), c->stream, r, err)
                         : hjr::device_bvh_build(c->dbvh, c->scene, pp.m.data(), pp.inv.data(), n_inst, (uint32_t)leaf_max, (uint32_t)opt_rounds,
                                                 f.lights.data(), f.lights.size(), c->stream, r, err);
    if (rc != HJR_OK) { set_error("hjr_set_transforms: " + err); return rc; }
    c->d_nodes.swap(c->dbvh.nodes); c->d_tri_geom.swap(c->dbvh.tri_geom); c->d_tri_shade.swap(c->dbvh.tri_shade);
    c->d_tri_inst.swap(c->dbvh.tri_inst); c->d_lights.swap(c->dbvh.lights);
    if (refit) { // the topology's
        f.n_nodes = c->frame.n_nodes; f.stack_need = c->frame.stack_need; f.depth = c->frame.depth;
        rf.count++;
        // the refit just made stays current; a tree that has grown past the guard is rebuilt at the next commit
        rf.rebuild = (double)r.sah > (double)rf.sah_full * (1.0 + c->opt.get(hjr::OPT_DEVICE_BVH_REFIT_GROWTH, 10) / 100.0);
    } else {
        f.n_nodes = r.n_nodes; f.stack_need = r.stack_need; f.depth = r.depth;
        rf.device = true; rf.rebuild = false; rf.count = 0; rf.tag = tag; rf.sah_full = r.sah;
    }
    rf.sah = r.sah;
    instances = r.instances;
    pp.build_ms = r.build_ms;
    return HJR_OK;
}

extern "C" int hjr_commit_transforms(hjr_ctx* c)
{
    if (!c) { set_error("hjr_commit_transforms: null context"); return HJR_ERR_ARG; }
    hjr_ctx::Prepared& pp = c->prep;
    if (!pp.valid) { set_error("hjr_commit_transforms: nothing prepared"); return HJR_ERR_STATE; }
    pp.valid = false;
    if (pp.same) {
        if (c->opt.get(hjr::OPT_VERBOSE, 0)) fprintf(stderr, "[hjr] transforms unchanged: frame data reused\n");
        return HJR_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    c->frame_gen++; // the frame data is replaced (a progressive frame cannot continue on it, even if the build below fails)
    uint32_t instances = 0; // option "device_bvh_instances": instance subtrees of this commit (0: an ordinary build)
    if (pp.key.device) {
        if (const int rc = commit_device(c, instances)) return rc;
        std::swap(c->frame, pp.frame);
    } else {
        std::swap(c->frame, pp.frame);
        c->refit = hjr_ctx::Refit(); // host-built data: nothing to refit
        c->dbvh.drop_topology();
        const hjr::FrameData& f = c->frame;
        bool ok = c->d_nodes.upload(f.nodes.data(), f.nodes.size() * 4, c->stream) &&
                  c->d_tri_geom.upload(f.tri_geom.data(), f.tri_geom.size() * 4, c->stream) &&
                  c->d_tri_shade.upload(f.tri_shade.data(), f.tri_shade.size() * 4, c->stream) &&
                  c->d_tri_inst.upload(f.tri_inst.data(), f.tri_inst.size() * 4, c->stream) &&
                  c->d_lights.upload(f.lights.data(), f.lights.size() * 4, c->stream);
        if (!ok) { c->have_frame = false; set_error("hjr_set_transforms: device upload failed"); return HJR_ERR_DEVICE; }
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    const hjr::FrameData& f = c->frame;
    c->have_frame = true;
    c->built.m.swap(pp.m); c->built.inv.swap(pp.inv); c->built.key = pp.key;
    c->stats.bvh_nodes = f.n_nodes;
    c->stats.bvh_depth = f.depth;
    c->stats.bvh_builder = pp.key.device ? 1u : 0u;
    c->stats.frame_build_ms = (float)pp.build_ms;
    c->stats.bvh_refits = c->refit.count;
    c->stats.bvh_sah = c->refit.sah;
    c->stats.bvh_instances = instances;
    if (instances) c->stats.bvh_topology_ms = c->dbvh.topo.ms;
    const bool refitted = pp.key.device && c->refit.count > 0;
    if (c->opt.get(hjr::OPT_VERBOSE, 0))
        fprintf(stderr, "[hjr] BVH%u (lds_mode %d): %u nodes (%zu KB), %u triangles (%zu KB), stack %u entries/lane, %s %s %.1f ms\n", f.width, f.lds_mode, f.n_nodes,
                (size_t)f.n_nodes * (f.width == 2 ? HJR_NODE2_F4 : HJR_NODE4_F4) * 16 / 1024, f.n_tris, (size_t)std::max(f.n_tris, 1u) * HJR_TRI_F4 * 16 / 1024,
                f.stack_need, pp.key.device ? "device" : "host", refitted ? "refit" : (instances ? (pp.key.graft ? "grafted instance build" : "instance build") : "build"), pp.build_ms);
    c->stats.n_triangles = f.n_tris;
    return HJR_OK;
}

// inspection copy of the current frame data (tests): synchronous, from the device buffers the kernels read
extern "C" int hjr_copy_frame_data(hjr_ctx* c, int what, void* dst, size_t dst_bytes, size_t* bytes)
{
    if (!c || !bytes) { set_error("hjr_copy_frame_data: null argument"); return HJR_ERR_ARG; }
    if (!c->have_frame) { set_error("hjr_copy_frame_data: no frame data (set transforms first)"); return HJR_ERR_STATE; }
    const hjr::FrameData& f = c->frame;
    const DevBuf* src = nullptr;
    size_t n = 0;
    switch (what) {
    case HJR_FRAME_NODES: src = &c->d_nodes; n = (size_t)f.n_nodes * (f.width == 2 ? HJR_NODE2_F4 : HJR_NODE4_F4) * 16; break;
    case HJR_FRAME_TRI_GEOM: src = &c->d_tri_geom; n = (size_t)std::max(f.n_tris, 1u) * HJR_TRI_F4 * 16; break;
    case HJR_FRAME_TRI_SHADE: src = &c->d_tri_shade; n = (size_t)f.n_tris * HJR_SHADE_F4 * 16; break;
    case HJR_FRAME_LIGHTS: src = &c->d_lights; n = (size_t)f.n_lights * HJR_LIGHT_F4 * 16; break;
    default: set_error("hjr_copy_frame_data: unknown HJR_FRAME_* value"); return HJR_ERR_ARG;
    }
    *bytes = n;
    if (!dst || n == 0) return HJR_OK;
    if (dst_bytes < n) { set_error("hjr_copy_frame_data: destination too small"); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(dst, src->p, n, hipMemcpyDeviceToHost));
    return HJR_OK;
}

extern "C" int hjr_set_transforms(hjr_ctx* c, const float* m, const float* inv, uint32_t n)
{
    const int rc = hjr_prepare_transforms(c, m, inv, n);
    return rc != HJR_OK ? rc : hjr_commit_transforms(c);
}

// hjr_set_lut / hjr_set_sky: an image of `texel` bytes per pixel into `buf`, its size into (cw, ch); a null or empty image switches it off
static int set_image(hjr_ctx* c, const char* who, DevBuf& buf, const void* rgba, int w, int h, size_t texel, int& cw, int& ch)
{
    HIPCHK(hipSetDevice(c->device));
    c->frame_gen++;
    c->tmp.have_prev = false; // temporal history: the shading / the lighting changes
    if (!rgba || w <= 0 || h <= 0) { cw = ch = 0; return HJR_OK; }
    if (!buf.upload(rgba, (size_t)w * (size_t)h * texel, c->stream)) { set_error(std::string(who) + ": upload failed"); return HJR_ERR_DEVICE; }
    HIPCHK(hipStreamSynchronize(c->stream));
    cw = w; ch = h;
    return HJR_OK;
}
extern "C" int hjr_set_lut(hjr_ctx* c, const uint8_t* rgba, int w, int h)
{
    if (!c) { set_error("hjr_set_lut: null context"); return HJR_ERR_ARG; }
    return set_image(c, "hjr_set_lut", c->d_lut, rgba, w, h, 4, c->lut_w, c->lut_h);
}
extern "C" int hjr_set_sky(hjr_ctx* c, const float* rgba, int w, int h)
{
    if (!c) { set_error("hjr_set_sky: null context"); return HJR_ERR_ARG; }
    return set_image(c, "hjr_set_sky", c->d_sky, rgba, w, h, 16, c->sky_w, c->sky_h);
}

// the render kernels live in their own translation units (hjr_launch.hip.h)
#ifndef HJR_LEAN_VARIANT
extern template int hjr_launch<HJR_INTEGRATOR_NEE, false>(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
extern template int hjr_launch<HJR_INTEGRATOR_NEE, true>(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
extern template int hjr_launch<HJR_INTEGRATOR_PT, false>(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
extern template int hjr_launch<HJR_INTEGRATOR_PT, true>(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
extern template int hjr_launch<HJR_INTEGRATOR_MIS, false>(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
extern template int hjr_launch<HJR_INTEGRATOR_MIS, true>(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
#endif
#if !defined(HJR_LEAN_VARIANT) && !defined(HJR_UNITY)
template <int I> int hjr_launch_fast(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t); // hjr_launch_fast_*.hip (HJR_FLAG_FAST_MATH)
extern template int hjr_launch_fast<HJR_INTEGRATOR_NEE>(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
extern template int hjr_launch_fast<HJR_INTEGRATOR_PT>(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
#define HJR_HAVE_FAST 1
#endif
#ifdef HJR_UNITY /* diagnostic variants (make variant): one translation unit, so that the __device__ diagnostic counters are one symbol */
#ifdef HJR_LEAN_VARIANT /* NEE without the statistics counters only; every other launch runs that kernel too (timing experiments, not pictures) */
template int hjr_launch<HJR_INTEGRATOR_NEE, false>(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
#else
#include "hjr_launch_nee.hip"
#include "hjr_launch_pt.hip"
#include "hjr_launch_mis.hip"
#include "hjr_launch_trace.hip"
#endif
#endif

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
static LaunchPlan plan_launch(const hjr_ctx* c, const KParams& kp, uint64_t n_items, int lds_mode, int integrator, bool fast)
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

// The samples one render call covers: the whole frame, or a sample pass of a progressive frame (include/henjou_hip.h)
struct PassRange {
    bool pass = false;         // a sample pass (else the whole frame, the one-shot launch sequence)
    uint32_t begin = 0, end = 0;
    uint32_t aovs = 0;         // AOVs requested: bit 0 colour, 1 albedo, 2 normal, 3 variance
};
static const uint32_t PASS_FLAGS = HJR_FLAG_PACKED | HJR_FLAG_ZERO_UNOWNED | HJR_FLAG_FAST_MATH; // the flags that change pixels
// options "firefly_clamp" > 0 and "firefly_clamp_passes" 1 (DESIGN.md §4 rule 10): a progressive frame keeps the colour chunk sums of all its passes
static bool firefly_keeps_chunks(const hjr_ctx* c) { return c->opt.get(hjr::OPT_FIREFLY_CLAMP, 0) > 0 && c->opt.get(hjr::OPT_FIREFLY_CLAMP_PASSES, 0) == 1; }

// The pass rules, checked before a call enqueues or writes anything: HJR_ERR_ARG for a bad range, HJR_ERR_STATE for a pass that does not
// continue the context's progressive frame.  Changes nothing; end_pass records a launch once it is enqueued.
static int check_pass(const hjr_ctx* c, const ParamsW* p, uint32_t aovs, PassRange& r)
{
    r = PassRange();
    r.aovs = aovs;
    if (p->sample_end == 0) {
        if (p->sample_begin != 0) { set_error("hjr_render: sample_begin without sample_end (sample_end 0 renders the whole frame)"); return HJR_ERR_ARG; }
        return HJR_OK;
    }
    if (p->spp == 0) { set_error("hjr_render: width, height and spp must be positive"); return HJR_ERR_ARG; }
    if (p->sample_begin == 0 && p->sample_end == p->spp) return HJR_OK; // the whole frame, through the same path
    if (c->opt.get(hjr::OPT_FIREFLY_CLAMP, 0) > 0 && !firefly_keeps_chunks(c)) { // the rule needs every chunk sum of a pixel; a progressive frame keeps running sums only
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

// this rank's share of a frame
struct FrameGeom {
    WorkRect rect; // the window, or else the frame: the extent everything below is derived from
    uint32_t world, tiles_x, chunk_spp, n_chunks;
    uint32_t chunk0, pass_chunks; // the chunks this launch renders: [chunk0, chunk0 + pass_chunks) (all n_chunks for a whole frame)
    uint64_t owned, n_items;
    int lds_mode; // LaunchPlan::lds_mode of the frame data
    PassRange pr;
};

// argument checks and tile geometry
static int frame_geometry(const hjr_ctx* c, const ParamsW* p, const void* d_color, const PassRange& pr, FrameGeom& g)
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
static void bind_scene_tables(const hjr_ctx* c, KParams& kp)
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
        const bool keep = g.pr.pass && firefly_keeps_chunks(c);
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
    bind_scene_tables(c, kp);
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
    LaunchPlan pl = plan_launch(c, kp, g.n_items, g.lds_mode, p->integrator, fast);
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
// ... after the render kernel, for every launch: sums of the sample chunks -> pixel means (a sample pass: -> running sums and running means;
// an adaptive one: statistic and stop decisions too, then the count of tiles still active goes to the host).  d_var: the variance AOV was
// requested (hjr_render_var); a frame of a single chunk has no chunk sums and gets the fill.
// the count of tiles still active goes to the host, behind the kernel that took the pass's stop decisions
static int adaptive_count(hjr_ctx* c, const FrameGeom& g, hipStream_t st)
{
    HIPCHK(hipMemcpyAsync(c->ad.h_active, (uint32_t*)c->ad.state.p + g.owned, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(c->ad.ready, st));
    return HJR_OK;
}
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
    return g.pr.pass && g.n_chunks > 1 && g.owned > 0 && firefly_keeps_chunks(c) && g.pr.end / g.chunk_spp >= 4u;
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
static int render_impl(hjr_ctx* c, const ParamsW* p, const PassRange& pr, void* d_color, void* d_albedo, void* d_normal, void* d_var, hipStream_t st, const void* d_prior = nullptr)
{
    FrameGeom g;
    KParams kp;
    int rc;
    if ((rc = frame_geometry(c, p, d_color, pr, g)) != HJR_OK) return rc;
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

static int fetch_stats(hjr_ctx* c, hipStream_t st)
{
    unsigned long long h[HJR_NSTAT];
    HIPCHK(hipMemcpyAsync(h, (char*)c->d_work.p + WorkArea::STATS, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t* dst = &c->stats.samples;
    for (int i = 0; i < 10; i++) dst[i] = h[i];
    c->stats.stack_overflow_pushes = h[10];
    { // option "firefly_clamp": the work area is zeroed before every launch, so a launch on which the rule did not act reads 0
        unsigned long long n = 0;
        HIPCHK(hipMemcpy(&n, (char*)c->d_work.p + WorkArea::FIREFLY, sizeof(n), hipMemcpyDeviceToHost));
        c->stats.firefly_clamped = n;
    }
    {
        unsigned long long nl[1 + HJR_NAN_LIST];
        HIPCHK(hipMemcpy(nl, (char*)c->d_work.p + WorkArea::NAN_LIST, sizeof(nl), hipMemcpyDeviceToHost));
        const uint32_t n = (uint32_t)std::min<unsigned long long>(nl[0], HJR_NAN_LIST);
        c->stats.nan_located = n;
        for (uint32_t i = 0; i < HJR_NAN_LIST; i++) {
            const unsigned long long k = i < n ? nl[1 + i] : 0ull;
            c->stats.nan_where[i][0] = (uint32_t)(k & 0x1fffu); c->stats.nan_where[i][1] = (uint32_t)((k >> 13) & 0x1fffu); c->stats.nan_where[i][2] = (uint32_t)(k >> 26);
        }
    }
#ifdef HJR_WF_TIMING
    { // diagnostic build only: where the waves of the wavefront kernel spend their clocks
        unsigned long long d[24];
        (void)hipMemcpyFromSymbol(d, HIP_SYMBOL(wf_diag), sizeof(d));
        const double tot = (double)d[0] + (double)d[1] + (double)d[2];
        if (tot > 0) {
            fprintf(stderr, "[hjr wf timing] scheduler idle %.1f%%  trace stage %.1f%% (hand-overs %.1f%%)  shade stage %.1f%% (waiting for context loads %.1f%%, store + push %.1f%%)\n",
                    100 * d[0] / tot, 100 * d[1] / tot, 100 * d[9] / tot, 100 * d[2] / tot, 100 * d[3] / tot, 100 * d[10] / tot);
            fprintf(stderr, "[hjr wf timing] shade batches %llu, %.1f contexts each; trace calls %llu, hand-overs %llu with %.1f finished rays each\n", d[4], d[4] ? (double)d[5] / d[4] : 0.0,
                    d[8], d[6], d[6] ? (double)d[7] / d[6] : 0.0);
            fprintf(stderr, "[hjr wf timing] trace stage lanes: outer iterations %llu with %.1f lanes holding a ray; node steps %llu wave-iterations x %.1f lanes; triangle tests %llu x %.1f lanes\n",
                    d[15], d[15] ? (double)d[16] / d[15] : 0.0, d[11], d[11] ? (double)d[12] / d[11] : 0.0, d[13], d[13] ? (double)d[14] / d[13] : 0.0);
            unsigned long long z[24] = { 0 };
            (void)hipMemcpyToSymbol(HIP_SYMBOL(wf_diag), z, sizeof(z));
        }
    }
#endif
#ifdef HJR_WF_WATCHDOG
    { // diagnostic build only: did the wavefront kernel run into its deadline, and where?
        unsigned long long wd[19];
        HIPCHK(hipMemcpy(wd, (char*)c->d_work.p + WorkArea::DIAG, sizeof(wd), hipMemcpyDeviceToHost));
        unsigned int where[8] = { 0 };
        (void)hipMemcpyFromSymbol(where, HIP_SYMBOL(wf_where), sizeof(where));
        if (where[1] | where[2] | where[3] | where[4] | where[5] | where[6]) {
            fprintf(stderr, "[hjr wf watchdog] deadline hit in (lane counts): take %u, push slot-wait %u, push publish-wait %u, trace loop %u, pop %u, scheduler %u\n", where[1], where[2], where[3], where[4], where[5], where[6]);
            fprintf(stderr, "[hjr wf watchdog] first workgroup to give up: block %llu live %llu items_held %llu\n", wd[17], wd[16], wd[18]);
            for (int q = 0; q < 5; q++) fprintf(stderr, "   queue %d: commit %llu head %llu tail %llu\n", q, wd[1 + q], wd[6 + q], wd[11 + q]);
            unsigned int zero[8] = { 0 };
            (void)hipMemcpyToSymbol(HIP_SYMBOL(wf_where), zero, sizeof(zero));
        }
    }
#endif
#ifdef HJR_TIMING
    { // diagnostic build only: wave-clock shares of the megakernel's loop phases and lane occupancies
        unsigned long long tk[25];
        HIPCHK(hipMemcpy(tk, (char*)c->d_work.p + WorkArea::DIAG, sizeof(tk), hipMemcpyDeviceToHost));
        const double tot = (double)tk[0] + (double)tk[1] + (double)tk[2];
        if (tot > 0) fprintf(stderr, "[hjr timing] roulette/refill/regeneration %.1f%%  fused trace %.1f%%  resolve + hit program + shading %.1f%%  (%.3g wave-clocks)\n",
                             100 * tk[0] / tot, 100 * tk[1] / tot, 100 * tk[2] / tot, tot);
        if (tk[3]) fprintf(stderr, "[hjr timing] lanes per round: closest-hit ray %.1f, shadow ray %.1f, serviced %.1f\n", (double)tk[4] / tk[3], (double)tk[5] / tk[3], (double)tk[6] / tk[3]);
        const unsigned long long* td = tk + 7;
        if (td[0]) fprintf(stderr, "[hjr timing] traversal: %.1f passes per round, %.1f lanes with a ray per pass (%.1f on a shadow ray); node steps %.2f wave-iterations per pass x %.1f lanes; "
                                   "leaf parts in %.0f%% of the passes x %.1f lanes; triangle tests %.2f wave-iterations per pass x %.1f lanes\n",
                           tk[3] ? (double)td[0] / tk[3] : 0.0, (double)td[1] / td[0], (double)td[8] / td[0], (double)td[2] / td[0], td[2] ? (double)td[3] / td[2] : 0.0,
                           100.0 * td[4] / td[0], td[4] ? (double)td[5] / td[4] : 0.0, (double)td[6] / td[0], td[6] ? (double)td[7] / td[6] : 0.0);
        const unsigned long long* ls = tk + 17; // (rounds that reach the site, rounds of those with at most 32 drawing lanes) x (light sample, Disney / glass sample, first walk step, roulette)
        if (tk[3]) fprintf(stderr, "[hjr timing] draw sites: rounds %llu light %llu %llu bsdf %llu %llu walk %llu %llu roulette %llu %llu\n", tk[3], ls[0], ls[1], ls[2], ls[3], ls[4], ls[5], ls[6], ls[7]);
    }
#endif
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
    if (const int rc = check_pass(c, p, (d_color ? 1u : 0u) | (d_albedo ? 2u : 0u) | (d_normal ? 4u : 0u) | (d_variance ? 8u : 0u), pr)) return rc;
    return render_impl(c, p, pr, d_color, d_albedo, d_normal, d_variance, stream_of(c, stream));
}
extern "C" int hjr_render_device(hjr_ctx* c, const hjr_params* p_user, void* d_color, void* d_albedo, void* d_normal, void* stream)
{
    return hjr_render_device_var(c, p_user, d_color, d_albedo, d_normal, nullptr, stream);
}

// the mode and size rules of every denoise entry point (include/henjou_hip.h: hjr_denoise)
static int denoise_check_sizes(int render_mode, uint32_t in_w, uint32_t in_h, uint32_t out_w, uint32_t out_h)
{
    if (in_w == 0 || in_h == 0 || in_w > 16384 || in_h > 16384) { set_error("hjr_denoise: bad input size"); return HJR_ERR_ARG; }
    const bool up = render_mode == HJR_MODE_DENOISE_UPSCALE2X;
    if (render_mode != HJR_MODE_DEFAULT && render_mode != HJR_MODE_DENOISE && !up) { set_error("hjr_denoise: unknown render mode"); return HJR_ERR_ARG; }
    if (!up && (out_w != in_w || out_h != in_h)) { set_error("hjr_denoise: output size must equal the input size in this mode"); return HJR_ERR_ARG; }
    if (up && (out_w / 2u != in_w || out_h / 2u != in_h)) { set_error("hjr_denoise: DenoiseUpScale2X renders at (out_w / 2, out_h / 2)"); return HJR_ERR_ARG; }
    return HJR_OK;
}

// OptixDenoiserManager::denoise() replacement (csrc/hjr_denoise.hip.h), device buffers, asynchronous on `hip_stream`
// `with_var`: the variance-guided variant (hjr_denoise_var_device), which also needs d_variance in the two Denoise modes
static int denoise_device_impl(hjr_ctx* c, int render_mode, uint32_t in_w, uint32_t in_h, const void* d_color, const void* d_albedo,
                               const void* d_normal, bool with_var, const void* d_variance, void* d_out, uint32_t out_w, uint32_t out_h, void* hip_stream)
{
    if (!c || !d_color || !d_out) { set_error("hjr_denoise: null argument"); return HJR_ERR_ARG; }
    if (const int rc = denoise_check_sizes(render_mode, in_w, in_h, out_w, out_h)) return rc;
    const bool up = render_mode == HJR_MODE_DENOISE_UPSCALE2X;
    if (render_mode != HJR_MODE_DEFAULT && (!d_albedo || !d_normal)) { set_error("hjr_denoise: the albedo and normal guide AOVs are required"); return HJR_ERR_ARG; }
    if (render_mode != HJR_MODE_DEFAULT && with_var && !d_variance) { set_error("hjr_denoise_var: the variance AOV is required"); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, hip_stream);
    const size_t in_bytes = (size_t)in_w * in_h * 16;
    if (render_mode == HJR_MODE_DEFAULT) { // blendFactor 1: the output is the input (denoiser.h:94-97)
        if (d_out != d_color) HIPCHK(hipMemcpyAsync(d_out, d_color, in_bytes, hipMemcpyDeviceToDevice, st));
        return HJR_OK;
    }
    if (!c->d_dn_a.reserve(in_bytes) || !c->d_dn_b.reserve(in_bytes)) { set_error("hjr_denoise: allocation failed"); return HJR_ERR_DEVICE; }
    if (with_var && (!c->d_dnv_a.reserve(in_bytes / 4) || !c->d_dnv_b.reserve(in_bytes / 4))) { set_error("hjr_denoise_var: allocation failed"); return HJR_ERR_DEVICE; }
    const dim3 block(256), grid = image_grid(in_w, in_h);
    const float4* src = (const float4*)d_color;
    float4* pp[2] = { (float4*)c->d_dn_a.p, (float4*)c->d_dn_b.p };
    const float* vsrc = (const float*)d_variance;
    float* vp[2] = { (float*)c->d_dnv_a.p, (float*)c->d_dnv_b.p };
    static decltype(&hjr_atrous_kernel<false>) const atrous[2] = { hjr_atrous_kernel<false>, hjr_atrous_kernel<true> }; // [with_var]
    for (int it = 0; it < HJR_ATROUS_PASSES; it++) {
        float4* dst = (!up && it == HJR_ATROUS_PASSES - 1) ? (float4*)d_out : pp[it & 1];
        // plain: the colour term is off, off, 1, 0.5, 0.25.  with_var: colour and variance ping-pong together, pass 0 clamps the variance it reads
        hipLaunchKernelGGL(atrous[with_var], grid, block, 0, st, src, vsrc, (const float4*)d_normal, (const float4*)d_albedo, dst, with_var ? vp[it & 1] : nullptr,
                           (int)in_w, (int)in_h, 1 << it, it == 0 ? 1 : 0, it < 2 ? 0.0f : 1.0f / (float)(1 << (it - 2)));
        if (with_var) vsrc = vp[it & 1];
        src = dst;
    }
    if (up) hipLaunchKernelGGL(hjr_upscale2x_kernel, image_grid(out_w, out_h), block, 0, st, src, (float4*)d_out, (int)in_w, (int)in_h, (int)out_w, (int)out_h);
    return launched();
}

extern "C" int hjr_denoise_device(hjr_ctx* c, int render_mode, uint32_t in_w, uint32_t in_h, const void* d_color, const void* d_albedo,
                                  const void* d_normal, void* d_out, uint32_t out_w, uint32_t out_h, void* hip_stream)
{
    return denoise_device_impl(c, render_mode, in_w, in_h, d_color, d_albedo, d_normal, false, nullptr, d_out, out_w, out_h, hip_stream);
}
extern "C" int hjr_denoise_var_device(hjr_ctx* c, int render_mode, uint32_t in_w, uint32_t in_h, const void* d_color, const void* d_albedo,
                                      const void* d_normal, const void* d_variance, void* d_out, uint32_t out_w, uint32_t out_h, void* hip_stream)
{
    return denoise_device_impl(c, render_mode, in_w, in_h, d_color, d_albedo, d_normal, true, d_variance, d_out, out_w, out_h, hip_stream);
}

// host-buffer form (what Renderer's frame loop does with AOV_Color / AOV_Albedo / AOV_Normal -> AOV_Output); synchronous
static int denoise_host_impl(hjr_ctx* c, int render_mode, uint32_t in_w, uint32_t in_h, const float* color, const float* albedo, const float* normal,
                             bool with_var, const float* variance, float* out, uint32_t out_w, uint32_t out_h)
{
    if (!c || !color || !out) { set_error("hjr_denoise: null argument"); return HJR_ERR_ARG; }
    if (in_w == 0 || in_h == 0 || out_w == 0 || out_h == 0) { set_error("hjr_denoise: empty image"); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const size_t in_bytes = (size_t)in_w * in_h * 16, out_bytes = (size_t)out_w * out_h * 16;
    if (!c->d_color.reserve(in_bytes) || !c->d_albedo.reserve(in_bytes) || !c->d_normal.reserve(in_bytes) || !c->d_dn_out.reserve(out_bytes)) {
        set_error("hjr_denoise: allocation failed");
        return HJR_ERR_DEVICE;
    }
    const bool var_in = with_var && variance;
    if (var_in && !c->d_variance.reserve(in_bytes / 4)) { set_error("hjr_denoise_var: allocation failed"); return HJR_ERR_DEVICE; }
    HostStage hs(c);
    hs.up(c->d_color.p, color, in_bytes);
    if (albedo) hs.up(c->d_albedo.p, albedo, in_bytes);
    if (normal) hs.up(c->d_normal.p, normal, in_bytes);
    if (var_in) hs.up(c->d_variance.p, variance, in_bytes / 4);
    // (the filter's own refusals come here, where they always did: finish() drains the uploads before it hands them on)
    if (hs.ok()) hs.rc = denoise_device_impl(c, render_mode, in_w, in_h, c->d_color.p, albedo ? c->d_albedo.p : nullptr, normal ? c->d_normal.p : nullptr,
                                             with_var, var_in ? c->d_variance.p : nullptr, c->d_dn_out.p, out_w, out_h, c->stream);
    hs.down(out, c->d_dn_out.p, out_bytes);
    return hs.finish(with_var ? "hjr_denoise_var" : "hjr_denoise");
}
extern "C" int hjr_denoise(hjr_ctx* c, int render_mode, uint32_t in_w, uint32_t in_h, const float* color, const float* albedo, const float* normal,
                           float* out, uint32_t out_w, uint32_t out_h)
{
    return denoise_host_impl(c, render_mode, in_w, in_h, color, albedo, normal, false, nullptr, out, out_w, out_h);
}
extern "C" int hjr_denoise_var(hjr_ctx* c, int render_mode, uint32_t in_w, uint32_t in_h, const float* color, const float* albedo, const float* normal,
                               const float* variance, float* out, uint32_t out_w, uint32_t out_h)
{
    return denoise_host_impl(c, render_mode, in_w, in_h, color, albedo, normal, true, variance, out, out_w, out_h);
}

// ---- spatial variance estimate (csrc/hjr_denoise.hip.h; include/henjou_hip.h: hjr_estimate_variance)
static int estimate_variance_check(const hjr_ctx* c, uint32_t w, uint32_t h, const void* color, const void* albedo, const void* normal, const void* variance_out)
{
    if (!c || !color || !variance_out) { set_error("hjr_estimate_variance: null argument"); return HJR_ERR_ARG; }
    if (w == 0 || h == 0 || w > 16384 || h > 16384) { set_error("hjr_estimate_variance: bad image size"); return HJR_ERR_ARG; }
    if (!albedo || !normal) { set_error("hjr_estimate_variance: the albedo and normal guide AOVs are required"); return HJR_ERR_ARG; }
    return HJR_OK;
}
// the kernel on device memory; the callers checked the arguments.  d_vin NULL = every pixel unknown; d_vout may be d_vin
static int estimate_variance_launch(uint32_t w, uint32_t h, const void* d_color, const void* d_albedo, const void* d_normal, const void* d_vin, void* d_vout, hipStream_t st)
{
    hipLaunchKernelGGL(hjr_spatial_var_kernel, image_grid(w, h), dim3(256), 0, st, (const float4*)d_color, (const float4*)d_normal, (const float4*)d_albedo,
                       (const float*)d_vin, (float*)d_vout, (int)w, (int)h);
    return launched();
}
extern "C" int hjr_estimate_variance_device(hjr_ctx* c, uint32_t w, uint32_t h, const void* d_color, const void* d_albedo, const void* d_normal, const void* d_variance_in,
                                            void* d_variance_out, void* hip_stream)
{
    if (const int rc = estimate_variance_check(c, w, h, d_color, d_albedo, d_normal, d_variance_out)) return rc;
    HIPCHK(hipSetDevice(c->device));
    return estimate_variance_launch(w, h, d_color, d_albedo, d_normal, d_variance_in, d_variance_out, stream_of(c, hip_stream));
}
extern "C" int hjr_estimate_variance(hjr_ctx* c, uint32_t w, uint32_t h, const float* color, const float* albedo, const float* normal, const float* variance_in,
                                     float* variance_out)
{
    if (const int rc = estimate_variance_check(c, w, h, color, albedo, normal, variance_out)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t bytes = (size_t)w * h * 16;
    if (!c->d_color.reserve(bytes) || !c->d_albedo.reserve(bytes) || !c->d_normal.reserve(bytes) || !c->d_variance.reserve(bytes / 4)) {
        set_error("hjr_estimate_variance: allocation failed");
        return HJR_ERR_DEVICE;
    }
    HostStage hs(c);
    hs.up(c->d_color.p, color, bytes);
    hs.up(c->d_albedo.p, albedo, bytes);
    hs.up(c->d_normal.p, normal, bytes);
    if (variance_in) hs.up(c->d_variance.p, variance_in, bytes / 4);
    if (hs.ok()) hs.rc = estimate_variance_launch(w, h, c->d_color.p, c->d_albedo.p, c->d_normal.p, variance_in ? c->d_variance.p : nullptr, c->d_variance.p, c->stream);
    hs.down(variance_out, c->d_variance.p, bytes / 4);
    return hs.finish("hjr_estimate_variance");
}

// ---- temporal accumulation with reprojection (csrc/hjr_temporal.hip.h; include/henjou_hip.h)
// The G-buffer pass's rules for the frame p describes, refused in the caller's words: `who` is the entry point, `t` what follows its name in
// each refusal: the pass's own texts, or those of an entry point that runs the pass for an option and checks ahead of its first enqueue.
#define HJR_GBUFFER_MAX_SIDE 8192
#define HJR_STR_(x) #x
#define HJR_STR(x) HJR_STR_(x)
#define HJR_GBUFFER_MAX_TEXT HJR_STR(HJR_GBUFFER_MAX_SIDE) " x " HJR_STR(HJR_GBUFFER_MAX_SIDE)
struct GbufTexts { const char *no_frame, *sharded, *too_large; };
static const GbufTexts GBUF_OWN = { ": no frame data (upload a scene and set transforms first)", ": world_size > 1 and HJR_FLAG_PACKED are not supported",
                                    ": frames larger than " HJR_GBUFFER_MAX_TEXT " are not supported" };
static const GbufTexts GBUF_TEMPORAL = { ": option \"denoise_temporal\" needs the frame data of this frame (upload a scene and set transforms first)",
                                         ": option \"denoise_temporal\" does not take world_size > 1 or HJR_FLAG_PACKED",
                                         ": option \"denoise_temporal\" does not take frames larger than " HJR_GBUFFER_MAX_TEXT };
static const GbufTexts GBUF_GUIDED = { ": option \"upscale_guided\" needs the frame data of this frame (upload a scene and set transforms first)",
                                       ": option \"upscale_guided\" does not take world_size > 1 or HJR_FLAG_PACKED",
                                       ": option \"upscale_guided\" does not take outputs larger than " HJR_GBUFFER_MAX_TEXT };
static int gbuffer_check(const hjr_ctx* c, const ParamsW* p, const std::string& who, const GbufTexts& t)
{
    if (!c->have_scene || !c->have_frame) { set_error(who + t.no_frame); return HJR_ERR_STATE; }
    if (p->world_size > 1 || (p->flags & HJR_FLAG_PACKED)) { set_error(who + t.sharded); return HJR_ERR_ARG; }
    if (p->width == 0 || p->height == 0) { set_error(who + ": empty image"); return HJR_ERR_ARG; }
    if (p->width > HJR_GBUFFER_MAX_SIDE || p->height > HJR_GBUFFER_MAX_SIDE) { set_error(who + t.too_large); return HJR_ERR_ARG; }
    return HJR_OK;
}
// G-buffer pass on device memory: the classifier's launch shape (one wave per tile, its stacks in dynamic LDS).  side 0: the plain pass;
// 2, 3, 4: the coverage pass with side x side sub-pixel rays
static int gbuffer_device_impl(hjr_ctx* c, const ParamsW* p, void* d_out, hipStream_t st, uint32_t side)
{
    if (!c || !p || !d_out) { set_error("hjr_render_gbuffer: null argument"); return HJR_ERR_ARG; }
    if (const int rc = refuse_window(p, "hjr_render_gbuffer")) return rc;
    if (const int rc = gbuffer_check(c, p, "hjr_render_gbuffer", GBUF_OWN)) return rc;
    HIPCHK(hipSetDevice(c->device));
    GbufArgs a;
    memset(&a, 0, sizeof(a));
    a.nodes = (const float4*)c->d_nodes.p; a.tri_geom = (const float4*)c->d_tri_geom.p; a.tri_inst = (const uint32_t*)c->d_tri_inst.p;
    a.tri_shade = (const uint32_t*)c->d_tri_shade.p; a.side = side;
    a.n_tris = c->frame.n_tris; a.width = p->width; a.height = p->height;
    a.tiles_x = (p->width + HJR_TILE - 1) / HJR_TILE;
    a.n_tiles = a.tiles_x * ((p->height + HJR_TILE - 1) / HJR_TILE);
    a.cam = p->camera;
    a.out = (hjr_gbuffer_px*)d_out;
    const unsigned grid = (unsigned)std::min<uint64_t>(a.n_tiles, (uint64_t)c->n_cus * 16);
    const size_t smem = (size_t)64 * c->frame.stack_need * 4;
    using Kernel = void (*)(GbufArgs);
    static const Kernel kernels[2][2] = { // [BVH4][coverage]
        { hjr_gbuffer_kernel<2, false>, hjr_gbuffer_kernel<2, true> },
        { hjr_gbuffer_kernel<4, false>, hjr_gbuffer_kernel<4, true> },
    };
    hipLaunchKernelGGL(kernels[c->frame.width != 2][side != 0], dim3(grid), dim3(64), smem, st, a);
    return launched();
}
static bool coverage_side_ok(uint32_t side)
{
    if (side >= 2 && side <= 4) return true;
    set_error("hjr_render_gbuffer_cov: side must be 2, 3 or 4");
    return false;
}
extern "C" int hjr_render_gbuffer_device(hjr_ctx* c, const hjr_params* p_user, void* d_out, void* hip_stream)
{
    ParamsW params; // sized struct (the long form: the render window behind hjr_params)
    if (!take_params(c, p_user, params, "hjr_render_gbuffer")) return HJR_ERR_ARG;
    return gbuffer_device_impl(c, &params, d_out, stream_of(c, hip_stream), 0);
}
extern "C" int hjr_render_gbuffer_cov_device(hjr_ctx* c, const hjr_params* p_user, uint32_t side, void* d_out, void* hip_stream)
{
    ParamsW params; // sized struct (the long form: the render window behind hjr_params)
    if (!coverage_side_ok(side)) return HJR_ERR_ARG;
    if (!take_params(c, p_user, params, "hjr_render_gbuffer_cov")) return HJR_ERR_ARG;
    return gbuffer_device_impl(c, &params, d_out, stream_of(c, hip_stream), side);
}
static int gbuffer_host_impl(hjr_ctx* c, const hjr_params* p_user, hjr_gbuffer_px* out, uint32_t side)
{
    ParamsW params; // sized struct (the long form: the render window behind hjr_params)
    if (!take_params(c, p_user, params, "hjr_render_gbuffer")) return HJR_ERR_ARG;
    if (!out) { set_error("hjr_render_gbuffer: null argument"); return HJR_ERR_ARG; }
    const size_t bytes = (size_t)params.width * params.height * sizeof(hjr_gbuffer_px);
    HostStage hs(c);
    if (bytes && !hs.buf.reserve(bytes)) { set_error("hjr_render_gbuffer: device allocation failed"); return HJR_ERR_DEVICE; }
    hs.rc = gbuffer_device_impl(c, &params, bytes ? hs.buf.p : (void*)out, c->stream, side); // (an empty image is the pass's refusal)
    hs.down(out, hs.buf.p, bytes);
    return hs.finish("hjr_render_gbuffer");
}
extern "C" int hjr_render_gbuffer(hjr_ctx* c, const hjr_params* p_user, hjr_gbuffer_px* out) { return gbuffer_host_impl(c, p_user, out, 0); }
extern "C" int hjr_render_gbuffer_cov(hjr_ctx* c, const hjr_params* p_user, uint32_t side, hjr_gbuffer_px* out)
{
    return coverage_side_ok(side) ? gbuffer_host_impl(c, p_user, out, side) : HJR_ERR_ARG;
}

// The accumulation kernel on device memory; the two frames were checked by the callers.  prev == nullptr: no previous frame (this is the
// one place that zeroes the missing side).  The records choose the kernel: out.response the windowed change test (a workgroup per
// 16 x 16 pixels), out.moments the temporal moments, a side's coverage rules 2' / 3'.
static int temporal_launch(hjr_ctx* c, const TemporalSide* prev, const TemporalSide& cur, uint32_t w, uint32_t h, uint32_t n_inst, const TemporalOut& out, hipStream_t st)
{
    TemporalArgs a;
    memset(&a, 0, sizeof(a));
    a.cur = cur; a.out = out;
    if (prev) { a.prev = *prev; a.have_prev = 1u; }
    a.width = w; a.height = h; a.n_instances = n_inst;
    a.n_tris = c->have_scene ? c->scene.n_triangles : 0xffffffffu; // prim ids are checked against the uploaded scene
    using Kernel = void (*)(TemporalArgs);
    static const Kernel kernels[2][2][2] = { // [response][a side carries coverage][moments]
        { { hjr_temporal_kernel<false, false>, hjr_temporal_kernel<false, true> }, { hjr_temporal_kernel<true, false>, hjr_temporal_kernel<true, true> } },
        { { hjr_temporal_resp_kernel<false, false>, hjr_temporal_resp_kernel<false, true> }, { hjr_temporal_resp_kernel<true, false>, hjr_temporal_resp_kernel<true, true> } },
    };
    const bool resp = out.response != nullptr;
    const dim3 grid = resp ? dim3((w + RESP_TILE - 1) / RESP_TILE, (h + RESP_TILE - 1) / RESP_TILE) : image_grid(w, h);
    hipLaunchKernelGGL(kernels[resp][a.prev.coverage || a.cur.coverage][out.moments != nullptr], grid, dim3(256), 0, st, a);
    return launched();
}
// argument checks of hjr_temporal_accumulate[_device]: the sized structs, sizes that agree, every pointer the kernel reads
// `prior`: hjr_temporal_prior[_device], which reads no colour or variance of the current frame: those two may be NULL
static int temporal_take(const hjr_temporal_frame* prev_user, const hjr_temporal_frame* cur_user, hjr_temporal_frame& prev, hjr_temporal_frame& cur, bool& have_prev, bool moments = false, const void* prev_moments = nullptr,
                         bool prior = false)
{
    if (!hjr::abi_take(cur_user, cur, "hjr_temporal_accumulate")) return HJR_ERR_ARG;
    have_prev = prev_user != nullptr;
    if (have_prev && !hjr::abi_take(prev_user, prev, "hjr_temporal_accumulate")) return HJR_ERR_ARG;
    if (cur.width == 0 || cur.height == 0 || cur.width > 16384 || cur.height > 16384) { set_error("hjr_temporal_accumulate: bad image size"); return HJR_ERR_ARG; }
    if (!cur.gbuffer || (!prior && (!cur.color || !cur.variance)) || (cur.n_instances && (!cur.transforms12 || !cur.inv_transforms12))) { set_error("hjr_temporal_accumulate: null pointer in the current frame"); return HJR_ERR_ARG; }
    if (have_prev) {
        if (prev.width != cur.width || prev.height != cur.height || prev.n_instances != cur.n_instances) { set_error("hjr_temporal_accumulate: width, height and n_instances of the two frames must agree"); return HJR_ERR_ARG; }
        if (!prev.gbuffer || !prev.color || !prev.variance || !prev.history || (prev.n_instances && (!prev.transforms12 || !prev.inv_transforms12))) { set_error("hjr_temporal_accumulate: null pointer in the previous frame"); return HJR_ERR_ARG; }
        if (moments && !prev_moments) { set_error("hjr_temporal_accumulate_moments: the previous frame has no moments"); return HJR_ERR_ARG; }
    }
    return HJR_OK;
}
// the kernel's view of a frame whose pointers are device pointers; d_moments: the frame's moments (read of a previous frame only)
static TemporalSide temporal_side(const hjr_temporal_frame& f, const void* d_moments)
{
    TemporalSide s;
    s.cam = f.camera; s.m = f.transforms12; s.inv = f.inv_transforms12; s.gbuf = f.gbuffer;
    s.color = (const float4*)f.color; s.variance = f.variance; s.history = f.history;
    s.moments = (const float2*)d_moments; s.coverage = f.coverage;
    return s;
}
// d_mom == nullptr: without moments, and d_prev_mom is not looked at; d_resp == nullptr: hjr_temporal_accumulate_moments_device
extern "C" int hjr_temporal_accumulate_response_device(hjr_ctx* c, const hjr_temporal_frame* prev_user, const hjr_temporal_frame* cur_user, void* d_color, void* d_var, void* d_hist,
                                                       const void* d_prev_mom, void* d_mom, void* d_resp, void* hip_stream)
{
    if (!c || !d_color || !d_var || !d_hist) { set_error("hjr_temporal_accumulate: null argument"); return HJR_ERR_ARG; }
    hjr_temporal_frame prev, cur;
    bool have_prev;
    if (const int rc = temporal_take(prev_user, cur_user, prev, cur, have_prev, d_mom != nullptr, d_prev_mom)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const TemporalSide ps = have_prev ? temporal_side(prev, d_prev_mom) : TemporalSide(), cs = temporal_side(cur, nullptr);
    const TemporalOut out = { (float4*)d_color, (float*)d_var, (float*)d_hist, (float2*)d_mom, (float*)d_resp };
    return temporal_launch(c, have_prev ? &ps : nullptr, cs, cur.width, cur.height, cur.n_instances, out, stream_of(c, hip_stream));
}
extern "C" int hjr_temporal_accumulate_moments_device(hjr_ctx* c, const hjr_temporal_frame* prev_user, const hjr_temporal_frame* cur_user, void* d_color, void* d_var, void* d_hist,
                                                      const void* d_prev_mom, void* d_mom, void* hip_stream)
{
    return hjr_temporal_accumulate_response_device(c, prev_user, cur_user, d_color, d_var, d_hist, d_prev_mom, d_mom, nullptr, hip_stream);
}
extern "C" int hjr_temporal_accumulate_device(hjr_ctx* c, const hjr_temporal_frame* prev_user, const hjr_temporal_frame* cur_user, void* d_color, void* d_var, void* d_hist, void* hip_stream)
{
    return hjr_temporal_accumulate_moments_device(c, prev_user, cur_user, d_color, d_var, d_hist, nullptr, nullptr, hip_stream);
}
// out_mom == nullptr: without moments, and prev_mom is not looked at; out_resp == nullptr: hjr_temporal_accumulate_moments
extern "C" int hjr_temporal_accumulate_response(hjr_ctx* c, const hjr_temporal_frame* prev_user, const hjr_temporal_frame* cur_user, float* out_color, float* out_var, float* out_hist,
                                                const float* prev_mom, float* out_mom, float* out_resp)
{
    if (!c || !out_color || !out_var || !out_hist) { set_error("hjr_temporal_accumulate: null argument"); return HJR_ERR_ARG; }
    hjr_temporal_frame f[2]; // [0] prev, [1] cur
    bool have_prev;
    if (const int rc = temporal_take(prev_user, cur_user, f[0], f[1], have_prev, out_mom != nullptr, prev_mom)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t npx = (size_t)f[1].width * f[1].height, nx = (size_t)f[1].n_instances * 48;
    const size_t mom = out_mom ? npx * 8 : 0, resp = out_resp ? npx * 4 : 0;
    // One temporary buffer behind one cursor: per side M, M^-1, the G-buffer, colour, variance (prev: history, moments), then the outputs.
    // Alignment: every image starts at a multiple of its element's (16 bytes for float4 and the records, 8 for float2, 4 for float).
    hjr_temporal_frame d[2]; // the staged copies: f[i] with device pointers
    const void* d_prev_mom = nullptr;
    TemporalOut out;
    const auto layout = [&](uintptr_t base) { // places every image from `base` on; returns the bytes that takes
        size_t at = 0;
        const auto take = [&](size_t bytes, size_t align) { const size_t o = (at + align - 1) & ~(align - 1); at = o + bytes; return (void*)(base + o); };
        for (int i = have_prev ? 0 : 1; i < 2; i++) {
            d[i] = f[i];
            d[i].transforms12 = (const float*)take(nx, 4); d[i].inv_transforms12 = (const float*)take(nx, 4);
            d[i].gbuffer = (const hjr_gbuffer_px*)take(npx * sizeof(hjr_gbuffer_px), 16);
            d[i].color = (const float*)take(npx * 16, 16); d[i].variance = (const float*)take(npx * 4, 4);
            d[i].history = i == 0 ? (const float*)take(npx * 4, 4) : nullptr;
            if (i == 0 && mom) d_prev_mom = take(mom, 8);
        }
        out.color = (float4*)take(npx * 16, 16); out.variance = (float*)take(npx * 4, 4); out.history = (float*)take(npx * 4, 4);
        out.moments = mom ? (float2*)take(mom, 8) : nullptr; out.response = resp ? (float*)take(resp, 4) : nullptr;
        return at;
    };
    HostStage hs(c);
    if (!hs.buf.reserve(layout(0))) { set_error("hjr_temporal_accumulate: device allocation failed"); return HJR_ERR_DEVICE; }
    layout((uintptr_t)hs.buf.p);
    for (int i = have_prev ? 0 : 1; i < 2; i++) {
        hs.up((void*)d[i].transforms12, f[i].transforms12, nx);
        hs.up((void*)d[i].inv_transforms12, f[i].inv_transforms12, nx);
        hs.up((void*)d[i].gbuffer, f[i].gbuffer, npx * sizeof(hjr_gbuffer_px));
        hs.up((void*)d[i].color, f[i].color, npx * 16);
        hs.up((void*)d[i].variance, f[i].variance, npx * 4);
        if (i == 0) hs.up((void*)d[i].history, f[i].history, npx * 4);
    }
    if (d_prev_mom) hs.up((void*)d_prev_mom, prev_mom, mom);
    const TemporalSide ps = have_prev ? temporal_side(d[0], d_prev_mom) : TemporalSide(), cs = temporal_side(d[1], nullptr);
    if (hs.ok()) hs.rc = temporal_launch(c, have_prev ? &ps : nullptr, cs, f[1].width, f[1].height, f[1].n_instances, out, c->stream);
    hs.down(out_color, out.color, npx * 16);
    hs.down(out_var, out.variance, npx * 4);
    hs.down(out_hist, out.history, npx * 4);
    hs.down(out_mom, out.moments, mom);
    hs.down(out_resp, out.response, resp);
    return hs.finish("hjr_temporal_accumulate");
}
extern "C" int hjr_temporal_accumulate_moments(hjr_ctx* c, const hjr_temporal_frame* prev_user, const hjr_temporal_frame* cur_user, float* out_color, float* out_var, float* out_hist,
                                               const float* prev_mom, float* out_mom)
{
    return hjr_temporal_accumulate_response(c, prev_user, cur_user, out_color, out_var, out_hist, prev_mom, out_mom, nullptr);
}
extern "C" int hjr_temporal_accumulate(hjr_ctx* c, const hjr_temporal_frame* prev_user, const hjr_temporal_frame* cur_user, float* out_color, float* out_var, float* out_hist)
{
    return hjr_temporal_accumulate_moments(c, prev_user, cur_user, out_color, out_var, out_hist, nullptr, nullptr);
}
extern "C" int hjr_temporal_reset(hjr_ctx* c)
{
    if (!c) { set_error("hjr_temporal_reset: null context"); return HJR_ERR_ARG; }
    c->tmp.have_prev = false;
    return HJR_OK;
}

// ---- the prior of adaptive sampling's rule 11 (csrc/hjr_temporal.hip.h section PRIOR; include/henjou_hip.h: hjr_temporal_prior)
// The kernel on device memory; prev == nullptr: no previous frame, every pixel (0, 0, 1, 0).  A side's coverage chooses rules 2' / 3'.
static int temporal_prior_launch(hjr_ctx* c, const TemporalSide* prev, const TemporalSide& cur, uint32_t w, uint32_t h, uint32_t n_inst, void* d_prior, hipStream_t st)
{
    TemporalArgs a;
    memset(&a, 0, sizeof(a));
    a.cur = cur;
    if (prev) { a.prev = *prev; a.have_prev = 1u; }
    a.width = w; a.height = h; a.n_instances = n_inst;
    a.n_tris = c->have_scene ? c->scene.n_triangles : 0xffffffffu; // as temporal_launch
    if (a.prev.coverage || a.cur.coverage) hipLaunchKernelGGL(hjr_temporal_prior_kernel<true>, image_grid(w, h), dim3(256), 0, st, a, (float4*)d_prior);
    else hipLaunchKernelGGL(hjr_temporal_prior_kernel<false>, image_grid(w, h), dim3(256), 0, st, a, (float4*)d_prior);
    return launched();
}
extern "C" int hjr_temporal_prior_device(hjr_ctx* c, const hjr_temporal_frame* prev_user, const hjr_temporal_frame* cur_user, void* d_prior, void* hip_stream)
{
    if (!c || !d_prior) { set_error("hjr_temporal_prior: null argument"); return HJR_ERR_ARG; }
    hjr_temporal_frame prev, cur;
    bool have_prev;
    if (const int rc = temporal_take(prev_user, cur_user, prev, cur, have_prev, false, nullptr, true)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const TemporalSide ps = have_prev ? temporal_side(prev, nullptr) : TemporalSide(), cs = temporal_side(cur, nullptr);
    return temporal_prior_launch(c, have_prev ? &ps : nullptr, cs, cur.width, cur.height, cur.n_instances, d_prior, stream_of(c, hip_stream));
}
extern "C" int hjr_temporal_prior(hjr_ctx* c, const hjr_temporal_frame* prev_user, const hjr_temporal_frame* cur_user, float* out_prior)
{
    if (!c || !out_prior) { set_error("hjr_temporal_prior: null argument"); return HJR_ERR_ARG; }
    hjr_temporal_frame f[2]; // [0] prev, [1] cur
    bool have_prev;
    if (const int rc = temporal_take(prev_user, cur_user, f[0], f[1], have_prev, false, nullptr, true)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t npx = (size_t)f[1].width * f[1].height, nx = (size_t)f[1].n_instances * 48;
    // one temporary buffer, 16-byte images first: the prior, per side the G-buffer (prev: and its colour), then the floats: per side M, M^-1 (prev: variance, history)
    hjr_temporal_frame d[2];
    char* d_prior = nullptr;
    const auto layout = [&](uintptr_t base) {
        size_t at = 0;
        const auto take = [&](size_t bytes) { char* const q = (char*)(base + at); at += bytes; return q; };
        d_prior = take(npx * 16);
        for (int i = have_prev ? 0 : 1; i < 2; i++) {
            d[i] = f[i];
            d[i].gbuffer = (const hjr_gbuffer_px*)take(npx * sizeof(hjr_gbuffer_px));
            d[i].color = i == 0 ? (const float*)take(npx * 16) : nullptr;
        }
        for (int i = have_prev ? 0 : 1; i < 2; i++) {
            d[i].transforms12 = (const float*)take(nx); d[i].inv_transforms12 = (const float*)take(nx);
            d[i].variance = i == 0 ? (const float*)take(npx * 4) : nullptr;
            d[i].history = i == 0 ? (const float*)take(npx * 4) : nullptr;
        }
        return at;
    };
    static_assert(sizeof(hjr_gbuffer_px) % 16 == 0, "the records keep the images behind them 16-byte aligned");
    HostStage hs(c);
    if (!hs.buf.reserve(layout(0))) { set_error("hjr_temporal_prior: device allocation failed"); return HJR_ERR_DEVICE; }
    layout((uintptr_t)hs.buf.p);
    for (int i = have_prev ? 0 : 1; i < 2; i++) {
        hs.up((void*)d[i].transforms12, f[i].transforms12, nx);
        hs.up((void*)d[i].inv_transforms12, f[i].inv_transforms12, nx);
        hs.up((void*)d[i].gbuffer, f[i].gbuffer, npx * sizeof(hjr_gbuffer_px));
        if (i == 0) {
            hs.up((void*)d[i].color, f[i].color, npx * 16);
            hs.up((void*)d[i].variance, f[i].variance, npx * 4);
            hs.up((void*)d[i].history, f[i].history, npx * 4);
        }
    }
    const TemporalSide ps = have_prev ? temporal_side(d[0], nullptr) : TemporalSide(), cs = temporal_side(d[1], nullptr);
    if (hs.ok()) hs.rc = temporal_prior_launch(c, have_prev ? &ps : nullptr, cs, f[1].width, f[1].height, f[1].n_instances, d_prior, c->stream);
    hs.down(out_prior, d_prior, npx * 16);
    return hs.finish("hjr_temporal_prior");
}

// Option "denoise_temporal", between the render (or the assembly of gathered shards) and the filter, all on `st`: G-buffer of this frame,
// a device copy of the transforms the current frame data was built from (`built`: what hjr_commit_transforms made current, so a
// frame loop that already prepares the next frame on another thread cannot be seen here), accumulation against the previous slot.
// `commit`: this call ends the frame (a whole-frame render, or the sample pass that ends at spp): the slots rotate.
// the current slot's buffers (no enqueue: post_plan calls it ahead of the first launch, temporal_stage again to no effect)
static int temporal_reserve(hjr_ctx* c, const ParamsW* p)
{
    hjr_ctx::Temporal& t = c->tmp;
    const size_t npx = (size_t)p->width * p->height, nx = c->built.m.size() * 4;
    hjr_ctx::Temporal::Slot& s = t.slot[t.cur];
    if (!s.color.reserve(npx * 16) || !s.variance.reserve(npx * 4) || !s.history.reserve(npx * 4) || !s.gbuf.reserve(npx * sizeof(hjr_gbuffer_px)) ||
        !s.xf.reserve(2 * nx + 16)) { set_error("hjr_render_denoised: temporal history allocation failed"); return HJR_ERR_DEVICE; }
    if (c->opt.get(hjr::OPT_DENOISE_TEMPORAL_MOMENTS, 0) && !s.moments.reserve(npx * 8)) { set_error("hjr_render_denoised: temporal history allocation failed"); return HJR_ERR_DEVICE; }
    if (c->opt.get(hjr::OPT_DENOISE_TEMPORAL_RESPONSE, 0) && !t.response.reserve(npx * 4)) { set_error("hjr_render_denoised: temporal history allocation failed"); return HJR_ERR_DEVICE; }
    if (c->opt.get(hjr::OPT_ADAPTIVE_TEMPORAL, 0) && !t.prior.reserve(npx * 16)) { set_error("hjr_render_denoised: temporal history allocation failed"); return HJR_ERR_DEVICE; }
    return HJR_OK;
}
// the history belongs to frames of this size, mode and instance count: anything else restarts
static void temporal_match(hjr_ctx* c, const ParamsW* p, int render_mode, uint32_t n_inst)
{
    hjr_ctx::Temporal& t = c->tmp;
    if (t.have_prev && (t.width != p->width || t.height != p->height || t.mode != render_mode || t.n_instances != n_inst)) t.have_prev = false;
}
// the current slot's G-buffer, transforms and camera of the frame p describes
static int temporal_trace(hjr_ctx* c, const ParamsW* p, uint32_t n_inst, uint32_t cov, hipStream_t st)
{
    hjr_ctx::Temporal::Slot& now = c->tmp.slot[c->tmp.cur];
    const size_t nx = (size_t)n_inst * 48;
    if (const int rc = gbuffer_device_impl(c, p, now.gbuf.p, st, cov)) return rc;
    if (nx) {
        HIPCHK(hipMemcpyAsync(now.xf.p, c->built.m.data(), nx, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync((char*)now.xf.p + nx, c->built.inv.data(), nx, hipMemcpyHostToDevice, st));
    }
    now.cam = p->camera;
    return HJR_OK;
}
// a slot as a frame of device pointers
static hjr_temporal_frame temporal_slot_frame(const hjr_ctx::Temporal::Slot& s, size_t nx, uint32_t cov)
{
    hjr_temporal_frame f = {};
    f.camera = s.cam; f.transforms12 = (const float*)s.xf.p; f.inv_transforms12 = (const float*)((const char*)s.xf.p + nx); f.gbuffer = (const hjr_gbuffer_px*)s.gbuf.p;
    f.color = (const float*)s.color.p; f.variance = (const float*)s.variance.p; f.history = (const float*)s.history.p; f.coverage = cov;
    return f;
}
// Option "adaptive_temporal", ahead of the render of a frame's first sample pass (the buffers stand: post_plan): the frame's G-buffer into the
// current slot and the prior against the committed history, for every pass of the frame.  Without a history there is no prior, and the frame
// is rule 6's.
static int temporal_prior_stage(hjr_ctx* c, const ParamsW* p, int render_mode, hipStream_t st)
{
    hjr_ctx::Temporal& t = c->tmp;
    const uint32_t n_inst = (uint32_t)(c->built.m.size() / 12);
    const size_t nx = (size_t)n_inst * 48;
    temporal_match(c, p, render_mode, n_inst);
    t.have_prior = false;
    if (!t.have_prev) return HJR_OK;
    const uint32_t cov = (uint32_t)c->opt.get(hjr::OPT_DENOISE_TEMPORAL_COVERAGE, 0);
    if (const int rc = temporal_trace(c, p, n_inst, cov, st)) return rc;
    const TemporalSide ps = temporal_side(temporal_slot_frame(t.slot[t.cur ^ 1], nx, cov), nullptr), cs = temporal_side(temporal_slot_frame(t.slot[t.cur], nx, cov), nullptr);
    if (const int rc = temporal_prior_launch(c, &ps, cs, p->width, p->height, n_inst, t.prior.p, st)) return rc;
    t.have_prior = true; t.prior_cur = t.cur;
    return HJR_OK;
}
// `commit` of temporal_stage: the frame in the current slot becomes the history, the slots rotate
static void temporal_commit(hjr_ctx* c, const ParamsW* p, int render_mode, uint32_t n_inst)
{
    hjr_ctx::Temporal& t = c->tmp;
    t.have_prev = true; t.width = p->width; t.height = p->height; t.mode = render_mode; t.n_instances = n_inst; t.cur ^= 1;
}
static int temporal_stage(hjr_ctx* c, const ParamsW* p, int render_mode, bool commit, const void*& d_color, const void*& d_var, hipStream_t st)
{
    hjr_ctx::Temporal& t = c->tmp;
    const uint32_t n_inst = (uint32_t)(c->built.m.size() / 12);
    temporal_match(c, p, render_mode, n_inst);
    const size_t nx = (size_t)n_inst * 48;
    if (const int rc = temporal_reserve(c, p)) return rc;
    hjr_ctx::Temporal::Slot &now = t.slot[t.cur], &before = t.slot[t.cur ^ 1];
    const uint32_t cov = (uint32_t)c->opt.get(hjr::OPT_DENOISE_TEMPORAL_COVERAGE, 0); // option "denoise_temporal_coverage": the coverage pass and rules 2' / 3' (setting it drops the history, so both slots agree)
    if (const int rc = temporal_trace(c, p, n_inst, cov, st)) return rc;
    const bool mom = c->opt.get(hjr::OPT_DENOISE_TEMPORAL_MOMENTS, 0) != 0; // option "denoise_temporal_moments": both slots carry (m1, m2) (setting it drops the history, so the previous slot has them)
    const bool resp = c->opt.get(hjr::OPT_DENOISE_TEMPORAL_RESPONSE, 0) != 0; // option "denoise_temporal_response": the windowed change test; its lambda image is written and not read again
    const auto frame_of = [&](const hjr_ctx::Temporal::Slot& s) { return temporal_slot_frame(s, nx, cov); };
    hjr_temporal_frame cur = frame_of(now);
    cur.color = (const float*)d_color; cur.variance = (const float*)d_var; cur.history = nullptr; // what was rendered: the slot's own images are the outputs
    const TemporalSide ps = temporal_side(frame_of(before), mom ? before.moments.p : nullptr), cs = temporal_side(cur, nullptr);
    const TemporalOut out = { (float4*)now.color.p, (float*)now.variance.p, (float*)now.history.p, mom ? (float2*)now.moments.p : nullptr, resp ? (float*)t.response.p : nullptr };
    if (const int rc = temporal_launch(c, t.have_prev ? &ps : nullptr, cs, p->width, p->height, n_inst, out, st)) return rc;
    d_color = now.color.p; d_var = now.variance.p;
    if (commit) temporal_commit(c, p, render_mode, n_inst);
    return HJR_OK;
}

// ---- guided 2x upscale (csrc/hjr_denoise.hip.h; include/henjou_hip.h: hjr_upscale_guided)
static int upscale_guided_check(const hjr_ctx* c, uint32_t in_w, uint32_t in_h, const void* color_lo, const void* gbuffer_lo, const hjr_camera* cam, const void* gbuffer_hi,
                                const void* out, uint32_t out_w, uint32_t out_h)
{
    if (!c || !color_lo || !gbuffer_lo || !cam || !gbuffer_hi || !out) { set_error("hjr_upscale_guided: null argument"); return HJR_ERR_ARG; }
    if (in_w == 0 || in_h == 0 || out_w == 0 || out_h == 0) { set_error("hjr_upscale_guided: empty image"); return HJR_ERR_ARG; }
    if (out_w / 2u != in_w || out_h / 2u != in_h) { set_error("hjr_upscale_guided: the input is (out_w / 2, out_h / 2)"); return HJR_ERR_ARG; }
    if (out_w > HJR_GBUFFER_MAX_SIDE || out_h > HJR_GBUFFER_MAX_SIDE) { set_error("hjr_upscale_guided: images larger than " HJR_GBUFFER_MAX_TEXT " are not supported"); return HJR_ERR_ARG; }
    return HJR_OK;
}
// the kernel on device memory; the callers checked the arguments
static int upscale_guided_launch(uint32_t in_w, uint32_t in_h, const void* d_color_lo, const void* d_gbuffer_lo, const hjr_camera& cam, const void* d_gbuffer_hi, void* d_out,
                                 uint32_t out_w, uint32_t out_h, hipStream_t st)
{
    hipLaunchKernelGGL(hjr_upscale_guided_kernel, image_grid(out_w, out_h), dim3(256), 0, st, (const float4*)d_color_lo, (const hjr_gbuffer_px*)d_gbuffer_lo,
                       (const hjr_gbuffer_px*)d_gbuffer_hi, (float4*)d_out, cam, (int)in_w, (int)in_h, (int)out_w, (int)out_h);
    return launched();
}
extern "C" int hjr_upscale_guided_device(hjr_ctx* c, uint32_t in_w, uint32_t in_h, const void* d_color_lo, const void* d_gbuffer_lo, const hjr_camera* cam,
                                         const void* d_gbuffer_hi, void* d_out, uint32_t out_w, uint32_t out_h, void* hip_stream)
{
    if (const int rc = upscale_guided_check(c, in_w, in_h, d_color_lo, d_gbuffer_lo, cam, d_gbuffer_hi, d_out, out_w, out_h)) return rc;
    HIPCHK(hipSetDevice(c->device));
    return upscale_guided_launch(in_w, in_h, d_color_lo, d_gbuffer_lo, *cam, d_gbuffer_hi, d_out, out_w, out_h, stream_of(c, hip_stream));
}
extern "C" int hjr_upscale_guided(hjr_ctx* c, uint32_t in_w, uint32_t in_h, const float* color_lo, const hjr_gbuffer_px* gbuffer_lo, const hjr_camera* cam,
                                  const hjr_gbuffer_px* gbuffer_hi, float* out, uint32_t out_w, uint32_t out_h)
{
    if (const int rc = upscale_guided_check(c, in_w, in_h, color_lo, gbuffer_lo, cam, gbuffer_hi, out, out_w, out_h)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t n_in = (size_t)in_w * in_h, n_out = (size_t)out_w * out_h;
    // one temporary buffer: [colour | output | low-resolution records | output-size records] (float4 images first: they stay 16-byte aligned)
    HostStage hs(c);
    if (!hs.buf.reserve((n_in + n_out) * (16 + sizeof(hjr_gbuffer_px)))) { set_error("hjr_upscale_guided: device allocation failed"); return HJR_ERR_DEVICE; }
    char* const d_color = (char*)hs.buf.p, *const d_out = d_color + n_in * 16, *const d_lo = d_out + n_out * 16, *const d_hi = d_lo + n_in * sizeof(hjr_gbuffer_px);
    hs.up(d_color, color_lo, n_in * 16);
    hs.up(d_lo, gbuffer_lo, n_in * sizeof(hjr_gbuffer_px));
    hs.up(d_hi, gbuffer_hi, n_out * sizeof(hjr_gbuffer_px));
    if (hs.ok()) hs.rc = upscale_guided_launch(in_w, in_h, d_color, d_lo, *cam, d_hi, d_out, out_w, out_h, c->stream);
    hs.down(out, d_out, n_out * 16);
    return hs.finish("hjr_upscale_guided");
}

// The post stage of a frame in a render mode, as hjr_render_denoised and hjr_denoise_shards_device (`who`) plan it ahead of their first
// enqueue and of any change to the progressive-frame state.
struct PostPlan {
    int mode;      // the render mode
    bool guides;   // not Default: the filter runs on the albedo and normal guides
    bool temporal; // option "denoise_temporal": accumulation over frames in front of the filter
    bool with_var; // option "denoise_variance" (or temporal): the variance AOV and the variance-guided filter
    bool guided;   // option "upscale_guided" in DenoiseUpScale2X: G-buffers and the guided upscale
};
static PostPlan post_options(const hjr_ctx* c, int render_mode)
{
    PostPlan pl;
    pl.mode = render_mode;
    pl.guides = render_mode != HJR_MODE_DEFAULT;
    pl.temporal = pl.guides && c->opt.get(hjr::OPT_DENOISE_TEMPORAL, 0) != 0;
    pl.with_var = pl.guides && (pl.temporal || c->opt.get(hjr::OPT_DENOISE_VARIANCE, 0) != 0);
    pl.guided = render_mode == HJR_MODE_DENOISE_UPSCALE2X && c->opt.get(hjr::OPT_UPSCALE_GUIDED, 0) != 0;
    return pl;
}
// Every refusal of the stage (world size / packed, the mode and size rules, the frame data and limits of the G-buffer passes), then every
// buffer it needs: the AOV staging, the filter's ping-pong colour and variance, the temporal slot, the guided upscale's G-buffers (the
// temporal stage traces the render-size one itself).  Nothing of the stage can fail behind the first launch but the runtime.
// `pr` non-null: the caller renders the frame itself (hjr_render_denoised), and the render's pass and argument rules speak where they
// always did, behind the guided upscale's and ahead of the filter's: *pr is the pass the render will run.
static int post_plan(hjr_ctx* c, const ParamsW* p, const PostPlan& pl, uint32_t out_w, uint32_t out_h, const char* who, PassRange* pr)
{
    const bool sharded = p->world_size > 1 || (p->flags & HJR_FLAG_PACKED);
    if (pl.temporal && sharded) { set_error(std::string(who) + GBUF_TEMPORAL.sharded); return HJR_ERR_ARG; }
    if (pl.guided && sharded) { set_error(std::string(who) + GBUF_GUIDED.sharded); return HJR_ERR_ARG; }
    if (pl.guided) {
        if (const int rc = denoise_check_sizes(pl.mode, p->width, p->height, out_w, out_h)) return rc;
        ParamsW hi = *p; // the second G-buffer pass
        hi.width = out_w; hi.height = out_h;
        if (const int rc = gbuffer_check(c, &hi, who, GBUF_GUIDED)) return rc;
    }
    if (pr) {
        FrameGeom g;
        if (const int rc = check_pass(c, p, (pl.guides ? 7u : 1u) | (pl.with_var ? 8u : 0u), *pr)) return rc;
        if (const int rc = frame_geometry(c, p, p, *pr, g)) return rc; // (no AOV buffer yet: any non-null pointer)
    }
    if (const int rc = denoise_check_sizes(pl.mode, p->width, p->height, out_w, out_h)) return rc;
    if (pl.temporal)
        if (const int rc = gbuffer_check(c, p, who, GBUF_TEMPORAL)) return rc;
    const size_t n_in = (size_t)p->width * p->height, n_out = (size_t)out_w * out_h;
    bool ok = c->d_color.reserve(n_in * 16);
    if (pl.guides) ok = ok && c->d_albedo.reserve(n_in * 16) && c->d_normal.reserve(n_in * 16) && c->d_dn_a.reserve(n_in * 16) && c->d_dn_b.reserve(n_in * 16);
    if (pl.with_var) ok = ok && c->d_variance.reserve(n_in * 4) && c->d_dnv_a.reserve(n_in * 4) && c->d_dnv_b.reserve(n_in * 4);
    if (pl.guided) ok = ok && (pl.temporal || c->d_ug_lo.reserve(n_in * sizeof(hjr_gbuffer_px))) && c->d_ug_hi.reserve(n_out * sizeof(hjr_gbuffer_px));
    if (!ok) { set_error(std::string(who) + ": allocation failed"); return HJR_ERR_DEVICE; }
    return pl.temporal ? temporal_reserve(c, p) : HJR_OK;
}

// What a frame in a render mode runs once its AOVs stand in the context's d_color / d_albedo / d_normal (/ d_variance), whether a render left
// them there (hjr_render_denoised) or the assembly of gathered shards (hjr_denoise_shards_device): the temporal stage if the option is on
// (`commit`: this call ends the frame), then the filter, plain or variance-guided, and the upscale of DenoiseUpScale2X.  All on `st`.
// Option "denoise_variance_spatial" with a variance in play: ahead of both, pixels of unknown variance get the spatial estimate, in place.
// pl.guided: the filter as in Denoise mode with its last pass into the ping-pong buffer, the G-buffer at the render size (the temporal
// stage's of this frame if there is one) and at the output size from the same camera, and the guided kernel in place of the bilinear one.
static int denoise_post_stage(hjr_ctx* c, const ParamsW* p, const PostPlan& pl, bool commit, void* d_out, uint32_t out_w, uint32_t out_h, hipStream_t st)
{
    const void *f_color = c->d_color.p, *f_var = pl.with_var ? c->d_variance.p : nullptr; // what the filter reads
    if (pl.with_var && c->opt.get(hjr::OPT_DENOISE_VARIANCE_SPATIAL, 0) != 0)
        if (const int rc = estimate_variance_launch(p->width, p->height, c->d_color.p, c->d_albedo.p, c->d_normal.p, c->d_variance.p, c->d_variance.p, st)) return rc;
    const int slot = c->tmp.cur; // the temporal stage's slot of this frame (a commit rotates the slots)
    if (pl.temporal)
        if (const int rc = temporal_stage(c, p, pl.mode, commit, f_color, f_var, st)) return rc;
    if (!pl.guided)
        return denoise_device_impl(c, pl.mode, p->width, p->height, f_color, pl.guides ? c->d_albedo.p : nullptr, pl.guides ? c->d_normal.p : nullptr, pl.with_var, f_var, d_out,
                                   out_w, out_h, st);
    void* const filtered = c->d_dn_a.p; // the last pass reads d_dn_b: the bilinear path's buffers
    if (const int rc = denoise_device_impl(c, HJR_MODE_DENOISE, p->width, p->height, f_color, c->d_albedo.p, c->d_normal.p, pl.with_var, f_var, filtered, p->width, p->height, st)) return rc;
    const void* g_lo = pl.temporal ? c->tmp.slot[slot].gbuf.p : c->d_ug_lo.p;
    if (!pl.temporal)
        if (const int rc = gbuffer_device_impl(c, p, c->d_ug_lo.p, st, 0)) return rc;
    ParamsW hi = *p;
    hi.width = out_w; hi.height = out_h;
    if (const int rc = gbuffer_device_impl(c, &hi, c->d_ug_hi.p, st, 0)) return rc;
    return upscale_guided_launch(p->width, p->height, filtered, g_lo, p->camera, c->d_ug_hi.p, d_out, out_w, out_h, st);
}

// One frame of Renderer's loop in a Denoise mode, on the device: optixLaunch -> denoise -> cpyGPUBufferToHost(AOV_Output)
// (renderer.h:1229-1281).  p->width x p->height is the RENDER size (already halved by the caller for DenoiseUpScale2X).
extern "C" int hjr_render_denoised(hjr_ctx* c, const hjr_params* p_user, int render_mode, float* out, uint32_t out_w, uint32_t out_h)
{
    ParamsW params; // sized struct (the long form: the render window behind hjr_params)
    if (!take_params(c, p_user, params, "hjr_render_denoised")) return HJR_ERR_ARG;
    const ParamsW* p = &params;
    if (!out) { set_error("hjr_render_denoised: null argument"); return HJR_ERR_ARG; }
    if (const int rc = refuse_window(p, "hjr_render_denoised")) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t in_bytes = (size_t)p->width * p->height * 16, out_bytes = (size_t)out_w * out_h * 16;
    if (in_bytes == 0 || out_bytes == 0) { set_error("hjr_render_denoised: empty image"); return HJR_ERR_ARG; }
    const PostPlan pl = post_options(c, render_mode);
    PassRange pr; // a sample pass: the running mean is filtered (a denoised preview; the last pass gives the one-shot call's image)
    if (const int rc = post_plan(c, p, pl, out_w, out_h, "hjr_render_denoised", &pr)) return rc;
    // Option "adaptive_temporal" is in effect on a sample pass of an adaptive frame in a Denoise mode with "denoise_temporal" on (DESIGN.md §4
    // rule 11): the frame's first pass computes the prior, rule 11 decides wherever there is one, and the pass that leaves no active tile
    // commits the history as the pass that ends at spp does.  Everywhere else nothing below differs from the call without the option.
    const bool at = pl.temporal && pr.pass && c->ad.threshold > 0.0f && c->opt.get(hjr::OPT_ADAPTIVE_TEMPORAL, 0) != 0;
    if (at && firefly_keeps_chunks(c)) {
        set_error("hjr_render_denoised: option \"adaptive_temporal\" cannot be combined with options \"firefly_clamp\" > 0 and \"firefly_clamp_passes\" 1: rule 10 and rule 11 would both take the stop decision");
        return HJR_ERR_ARG;
    }
    if (!c->d_dn_out.reserve(out_bytes)) { set_error("hjr_render_denoised: allocation failed"); return HJR_ERR_DEVICE; }
    if (pl.with_var) HIPCHK(hipMemsetAsync(c->d_variance.p, 0, in_bytes / 4, c->stream));
    HIPCHK(hipMemsetAsync(c->d_color.p, 0, in_bytes, c->stream));
    if (pl.guides) { HIPCHK(hipMemsetAsync(c->d_albedo.p, 0, in_bytes, c->stream)); HIPCHK(hipMemsetAsync(c->d_normal.p, 0, in_bytes, c->stream)); }
    HostStage hs(c);
    if (at && pr.begin == 0) hs.rc = temporal_prior_stage(c, p, render_mode, c->stream);
    // a continuing pass reuses its frame's prior while the history it was gathered from stands
    const void* const d_prior = at && c->tmp.have_prior && c->tmp.have_prev && c->tmp.prior_cur == c->tmp.cur ? c->tmp.prior.p : nullptr;
    const bool last = !pr.pass || pr.end == p->spp;
    if (hs.ok()) hs.rc = render_impl(c, p, pr, c->d_color.p, pl.guides ? c->d_albedo.p : nullptr, pl.guides ? c->d_normal.p : nullptr, pl.with_var ? c->d_variance.p : nullptr, c->stream, d_prior);
    if (hs.ok()) hs.rc = denoise_post_stage(c, p, pl, last, c->d_dn_out.p, out_w, out_h, c->stream);
    hs.down(out, c->d_dn_out.p, out_bytes);
    const int rc = hs.finish("hjr_render_denoised");
    // (the stream is drained: the count the pass read back is at hand)  No tile is left: the frame is over, its accumulation is the history
    if (rc == HJR_OK && at && !last && c->ad.frame && *c->ad.h_active == 0u) {
        temporal_commit(c, p, render_mode, (uint32_t)(c->built.m.size() / 12));
        c->pass.active = false; c->pass.committed = true;
    }
    return rc;
}

// ---- gathered shards of a multi-GPU frame (include/henjou_hip.h; kernel: csrc/hjr_aux.hip.h)
static int assemble_launch(const hjr_shards& s, uint32_t w, uint32_t h, void* d_color, void* d_albedo, void* d_normal, void* d_variance, hipStream_t st)
{
    ShardArgs a;
    memset(&a, 0, sizeof(a));
    a.color = (const char*)s.color; a.albedo = (const char*)s.albedo; a.normal = (const char*)s.normal; a.variance = (const char*)s.variance;
    a.out_color = (float4*)d_color; a.out_albedo = (float4*)d_albedo; a.out_normal = (float4*)d_normal; a.out_variance = (float*)d_variance;
    a.rank_stride = s.rank_stride; a.width = w; a.height = h; a.world = s.world_size;
    a.tiles_x = (w + HJR_TILE - 1) / HJR_TILE;
    hipLaunchKernelGGL(hjr_assemble_shards_kernel, dim3((a.tiles_x + 3u) / 4u, (h + HJR_TILE - 1) / HJR_TILE), dim3(256), 0, st, a);
    return launched();
}
extern "C" int hjr_assemble_shards_device(hjr_ctx* c, const hjr_shards* shards, uint32_t w, uint32_t h, void* d_color, void* d_albedo, void* d_normal, void* d_variance,
                                          void* hip_stream)
{
    if (!c) { set_error("hjr_assemble_shards_device: null context"); return HJR_ERR_ARG; }
    hjr_shards s;
    const void* const out[4] = { d_color, d_albedo, d_normal, d_variance };
    if (!hjr::abi_take(shards, s, "hjr_assemble_shards_device")) return HJR_ERR_ARG;
    if (const int rc = hjr::check_shards(s, w, h, out, "hjr_assemble_shards_device")) return rc;
    HIPCHK(hipSetDevice(c->device));
    return assemble_launch(s, w, h, d_color, d_albedo, d_normal, d_variance, stream_of(c, hip_stream));
}
// Rank 0's half of a multi-GPU frame in a Denoise mode: the gathered blocks -> the context's AOV buffers -> the post stage of hjr_render_denoised.
// Every argument and state check comes before the first enqueue.
extern "C" int hjr_denoise_shards_device(hjr_ctx* c, const hjr_params* p_user, int render_mode, const hjr_shards* gathered, void* d_out, uint32_t out_w, uint32_t out_h,
                                         void* hip_stream)
{
    ParamsW params; // sized struct (the long form: the render window behind hjr_params)
    if (!take_params(c, p_user, params, "hjr_denoise_shards_device")) return HJR_ERR_ARG;
    if (!d_out) { set_error("hjr_denoise_shards_device: null argument"); return HJR_ERR_ARG; }
    if (const int rc = refuse_window(&params, "hjr_denoise_shards_device")) return rc;
    if (render_mode == HJR_MODE_DEFAULT) { set_error("hjr_denoise_shards_device: Render_mode Default has no filter (hjr_assemble_shards_device assembles the frame)"); return HJR_ERR_ARG; }
    params.rank = 0; params.world_size = 1; params.flags &= ~HJR_FLAG_PACKED; // `frame` describes the whole frame; gathered->world_size is how it was rendered
    const ParamsW* p = &params;
    if (const int rc = denoise_check_sizes(render_mode, p->width, p->height, out_w, out_h)) return rc;
    const bool whole = p->sample_end == 0 || (p->sample_begin == 0 && p->sample_end == p->spp);
    if (!whole && (p->sample_begin >= p->sample_end || p->sample_end > p->spp)) { set_error("hjr_denoise_shards_device: bad sample range"); return HJR_ERR_ARG; }
    const PostPlan pl = post_options(c, render_mode);
    hjr_shards s; // sized struct
    if (!hjr::abi_take(gathered, s, "hjr_denoise_shards_device")) return HJR_ERR_ARG;
    if (!s.color || !s.albedo || !s.normal) { set_error("hjr_denoise_shards_device: the colour, albedo and normal blocks are required"); return HJR_ERR_ARG; }
    if (pl.with_var && !s.variance) { set_error("hjr_denoise_shards_device: options \"denoise_variance\" / \"denoise_temporal\" need the variance block"); return HJR_ERR_ARG; }
    if (!pl.with_var) s.variance = nullptr; // a block the filter does not read stays where it is
    HIPCHK(hipSetDevice(c->device));
    if (const int rc = post_plan(c, p, pl, out_w, out_h, "hjr_denoise_shards_device", nullptr)) return rc;
    const void* const out[4] = { c->d_color.p, c->d_albedo.p, c->d_normal.p, pl.with_var ? c->d_variance.p : nullptr };
    if (const int rc = hjr::check_shards(s, p->width, p->height, out, "hjr_denoise_shards_device")) return rc;
    hipStream_t st = stream_of(c, hip_stream);
    if (const int rc = assemble_launch(s, p->width, p->height, c->d_color.p, c->d_albedo.p, c->d_normal.p, pl.with_var ? c->d_variance.p : nullptr, st)) return rc;
    return denoise_post_stage(c, p, pl, whole || p->sample_end == p->spp, d_out, out_w, out_h, st);
}

// Round-trips every child ref the builder can emit for a tree that host/frame.cpp admits to the 16-bit-stack layout
// (inner node ids < HJR_STACK16_MAX_NODES; leaves of 0..HJR_STACK16_LEAF_MAX triangles starting below HJR_STACK16_MAX_TRIS)
// through stack_enc<uint16_t> / stack_dec.  Pure host code (the same inline functions the kernel uses); 0 = all refs survive.
extern "C" int hjr_selftest_stack16(void)
{
    for (uint32_t n = 0; n < HJR_STACK16_MAX_NODES; n++)
        if (stack_dec(stack_enc<uint16_t>(n)) != n) return 1;
    for (uint32_t count = 0; count <= HJR_STACK16_LEAF_MAX; count++)
        for (uint32_t first = 0; first < HJR_STACK16_MAX_TRIS; first++) {
            const uint32_t ref = HJR_LEAF_FLAG | (count << 27) | first;
            if (stack_dec(stack_enc<uint16_t>(ref)) != ref) return 2;
        }
    return 0;
}

// Ray-batch test hook (include/henjou_hip.h; kernels: csrc/hjr_trace_hook.hip.h).  The layout is plan_launch's for a megakernel render of the
// current frame data under the context's options; the rays, the results and two counters share one temporary buffer.
extern "C" int hjr_trace_rays(hjr_ctx* c, int path, uint32_t n, const hjr_ray* shadow, const hjr_ray* closest, hjr_ray_result* out)
{
    const int loop = path & ~(int)HJR_TRACE_FAST_BUILD;
    const bool fast = (path & HJR_TRACE_FAST_BUILD) != 0;
    if (loop == HJR_TRACE_WAVEFRONT) { set_error("hjr_trace_rays: HJR_TRACE_WAVEFRONT is not built (the wavefront trace stage cannot be handed independent rays; include/henjou_hip.h)"); return HJR_ERR_ARG; }
    if (loop != HJR_TRACE_STANDALONE && loop != HJR_TRACE_FUSED) { set_error("hjr_trace_rays: unknown path"); return HJR_ERR_ARG; }
    if (n && (!shadow || !closest || !out)) { set_error("hjr_trace_rays: null ray or result pointer"); return HJR_ERR_ARG; }
    if (n > (1u << 24)) { set_error("hjr_trace_rays: more than 2^24 pairs in one call"); return HJR_ERR_ARG; }
    if (!c) { set_error("hjr_trace_rays: null context"); return HJR_ERR_ARG; }
    if (!c->have_scene || !c->have_frame) { set_error("hjr_trace_rays: no frame data (upload a scene and set transforms first)"); return HJR_ERR_STATE; }
#ifdef HJR_LEAN_VARIANT /* the lean experiment build instantiates the NEE megakernel only: no hook kernels */
    (void)fast;
    set_error("hjr_trace_rays: the lean experiment build has no ray-batch kernels");
    return HJR_ERR_ARG;
#else
#ifndef HJR_HAVE_FAST
    if (fast) { set_error("hjr_trace_rays: this build has no HJR_TRACE_FAST_BUILD kernels"); return HJR_ERR_ARG; }
#endif
    if (n == 0) return HJR_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    KParams kp;
    memset(&kp, 0, sizeof(kp));
    bind_scene_tables(c, kp);
    const int lds_mode = launch_layout(c->frame);
    // (`fast` of plan_launch = "megakernel family whatever option pipeline says": the hook has no wavefront path)
    const LaunchPlan pl = plan_launch(c, kp, n, lds_mode, HJR_INTEGRATOR_NEE, true);
    const size_t rays = (size_t)n * sizeof(hjr_ray);
    HostStage hs(c);
    if (!hs.buf.reserve(64 + 3 * rays)) { set_error("hjr_trace_rays: device allocation failed"); return HJR_ERR_DEVICE; }
    char* const base = (char*)hs.buf.p;
    TraceArgs a;
    memset(&a, 0, sizeof(a));
    a.next = (unsigned int*)base; a.n_over = (unsigned long long*)(base + 8);
    a.shadow = (const hjr_ray*)(base + 64); a.closest = (const hjr_ray*)(base + 64 + rays); a.out = (hjr_ray_result*)(base + 64 + 2 * rays);
    a.n = n; a.round_cap = 2u * n + 64u;
    std::vector<hjr_ray_result> init(n);
    memset(init.data(), 0, rays);
    for (uint32_t i = 0; i < n; i++) { init[i].prim = 0xffffffffu; init[i].status = HJR_TRACE_STATUS_UNTRACED; }
    unsigned long long n_over = 0;
    hs.e = hipMemsetAsync(base, 0, 64, c->stream);
    hs.up(base + 64, shadow, rays);
    hs.up(base + 64 + rays, closest, rays);
    hs.up(base + 64 + 2 * rays, init.data(), rays);
    if (hs.ok()) {
#ifdef HJR_HAVE_FAST
        hs.rc = fast ? hjr_launch_trace_fast(c, pl, loop == HJR_TRACE_FUSED, a, c->stream) : hjr_launch_trace(c, pl, loop == HJR_TRACE_FUSED, a, c->stream);
#else
        hs.rc = hjr_launch_trace(c, pl, loop == HJR_TRACE_FUSED, a, c->stream);
#endif
        if (hs.rc == HJR_OK) hs.e = hipGetLastError();
    }
    hs.down(out, base + 64 + 2 * rays, rays);
    hs.down(&n_over, base + 8, 8);
    if (const int rc = hs.finish("hjr_trace_rays")) return rc;
    if (c->event_pending) { hjr_stats prev; memset(&prev, 0, sizeof(prev)); prev.struct_size = (uint32_t)sizeof(prev); (void)hjr_get_stats(c, &prev); } // counters of an earlier render land first
    c->stats.lds_mode = (uint32_t)lds_mode; c->stats.stack_need = c->frame.stack_need; c->stats.stack_lds_entries = pl.kp.stack_lds_entries;
    c->stats.stack_overflow_pushes = n_over;
    return HJR_OK;
#endif
}

// hjr_pack_tiles_device / hjr_unpack_tiles_device: the two kernels take (source, destination) and are otherwise one launch
static int tiles_device(hjr_ctx* c, bool pack, const void* d_frame, const void* d_packed, uint32_t w, uint32_t h, uint32_t rank, uint32_t world, void* hip_stream)
{
    if (!c || !d_frame || !d_packed || w == 0 || h == 0 || world == 0 || rank >= world) { set_error(std::string(pack ? "hjr_pack_tiles_device" : "hjr_unpack_tiles_device") + ": bad argument"); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const uint32_t n = hjr_owned_tiles(w, h, rank, world);
    if (n == 0) return HJR_OK;
    hipLaunchKernelGGL(pack ? hjr_pack_tiles_kernel : hjr_unpack_tiles_kernel, dim3((unsigned)(((size_t)n * 64 + 255) / 256)), dim3(256), 0, stream_of(c, hip_stream),
                       (const float4*)(pack ? d_frame : d_packed), (float4*)(pack ? d_packed : d_frame), w, h, (w + HJR_TILE - 1) / HJR_TILE, n, rank, world);
    return launched();
}
extern "C" int hjr_pack_tiles_device(hjr_ctx* c, const void* d_frame, uint32_t w, uint32_t h, uint32_t rank, uint32_t world, void* d_packed, void* hip_stream)
{
    return tiles_device(c, true, d_frame, d_packed, w, h, rank, world, hip_stream);
}
extern "C" int hjr_unpack_tiles_device(hjr_ctx* c, const void* d_packed, uint32_t w, uint32_t h, uint32_t rank, uint32_t world, void* d_frame, void* hip_stream)
{
    return tiles_device(c, false, d_frame, d_packed, w, h, rank, world, hip_stream);
}

// hjr_render_file's bucketed frames (host/render_file.cpp is plain host code): the context's two buffers, and the frame's one download
namespace hjr {
int bucket_buffer(hjr_ctx* c, int slot, size_t bytes, void** d_out)
{
    if (!c || !d_out || slot < 0 || slot > 1) { set_error("bucket_buffer: bad argument"); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    if (!c->d_bucket[slot].reserve(bytes)) { set_error("hjr_render_file: bucket buffer allocation failed"); return HJR_ERR_DEVICE; }
    *d_out = c->d_bucket[slot].p;
    return HJR_OK;
}
int bucket_download(hjr_ctx* c, float* host, const void* d_frame, size_t bytes)
{
    if (!c || !host || !d_frame) { set_error("bucket_download: null argument"); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(host, d_frame, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return HJR_OK;
}
} // namespace hjr

// hjr_blit_window_device: a window launch's float4 image into its rectangle of a full-size frame (csrc/hjr_aux.hip.h)
extern "C" int hjr_blit_window_device(hjr_ctx* c, const void* d_window, const uint32_t window[4], void* d_frame, uint32_t w, uint32_t h, void* hip_stream)
{
    if (!c || !d_window || !window || !d_frame) { set_error("hjr_blit_window_device: null argument"); return HJR_ERR_ARG; }
    if (const int rc = hjr::check_blit_window(window, w, h, "hjr_blit_window_device")) return rc;
    HIPCHK(hipSetDevice(c->device));
    const uint32_t ww = window[2] - window[0], wh = window[3] - window[1];
    hipLaunchKernelGGL(hjr_blit_window_kernel, image_grid(ww, wh), dim3(256), 0, stream_of(c, hip_stream), (const float4*)d_window, (float4*)d_frame, window[0], window[1], ww, wh, w);
    return launched();
}

extern "C" int hjr_preview_device(hjr_ctx* c, const void* d_color, uint32_t w, uint32_t h, int tonemap, void* d_rgba8, void* hip_stream)
{
    if (!c || !d_color || !d_rgba8 || w == 0 || h == 0 || tonemap < HJR_TONEMAP_NONE || tonemap > HJR_TONEMAP_ACES) { set_error("hjr_preview_device: bad argument"); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, hip_stream);
    const size_t n = (size_t)w * h;
    hipLaunchKernelGGL(hjr_preview_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float4*)d_color, (uchar4*)d_rgba8, n, tonemap);
    return launched();
}

extern "C" int hjr_synchronize(hjr_ctx* c)
{
    if (!c) { set_error("hjr_synchronize: null context"); return HJR_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    return HJR_OK;
}

extern "C" int hjr_get_stats(hjr_ctx* c, hjr_stats* out)
{
    if (!c || !out) { set_error("hjr_get_stats: null argument"); return HJR_ERR_ARG; }
    uint32_t out_size;
    if (!hjr::abi_size(out, out_size, "hjr_get_stats")) return HJR_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (c->event_pending) {
        HIPCHK(hipEventSynchronize(c->ev1));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        c->stats.last_kernel_ms = ms;
        c->event_pending = false;
        if (c->d_work.p) { int rc = fetch_stats(c, c->stream); if (rc != HJR_OK) return rc; }
    }
    return hjr::abi_give(out, c->stats, "hjr_get_stats") ? HJR_OK : HJR_ERR_ARG; // sized struct: at most out->struct_size bytes are written
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
    if (const int rc = check_pass(c, p, 1u | (albedo ? 2u : 0u) | (normal ? 4u : 0u) | (variance ? 8u : 0u), pr)) return rc;
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
    hs.rc = render_impl(c, p, pr, c->d_color.p, albedo ? c->d_albedo.p : nullptr, normal ? c->d_normal.p : nullptr, variance ? c->d_variance.p : nullptr, c->stream);
    for (int i = 0; i < 4; i++)
        if (host[i]) hs.down(host[i], bufs[i]->p, len[i]);
    return hs.finish("hjr_render"); // drains the stream: CUDA_SYNC_CHECK (renderer.h:1242)
}
extern "C" int hjr_render(hjr_ctx* c, const hjr_params* p_user, float* color, float* albedo, float* normal)
{
    return hjr_render_var(c, p_user, color, albedo, normal, nullptr);
}
