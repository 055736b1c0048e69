// What the device-layer units (hjr_device.hip, hjr_render.hip, hjr_post.hip, hjr_util.hip) share: the error and launch helpers, the sized
// parameters and the work rectangle of a render call, the host-buffer stage, and the few functions one unit calls in another.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hjr_context.h"
#include "../host/abi.hpp"
#pragma GCC visibility push(hidden) /* to the end of this header: what the units share is the library's own, no exported name */
#include "../host/stage_layout.hpp"

#if !defined(HJR_LEAN_VARIANT) && !defined(HJR_UNITY)
#define HJR_HAVE_FAST 1 /* the approximate-arithmetic units hjr_launch_fast_*.hip are linked (HJR_FLAG_FAST_MATH, HJR_TRACE_FAST_BUILD) */
#endif

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
// such entry point returns while a copy it enqueued is in flight, and folds the first error.
// An entry point that stages through a context-owned buffer calls up() / down() itself.  One that stages through none states each image once:
// add(device pointer, host source or null, host destination or null, bytes, alignment) (host/stage_layout.hpp); place() reserves `buf` for
// all of them, sets the pointers and enqueues the uploads, fetch() the downloads behind the launch.  `buf` is released behind the drain only.
struct HostStage : hjr::StageLayout {
    hjr_ctx* c;
    DevBuf buf;
    int rc = HJR_OK;           // of the launch
    hipError_t e = hipSuccess; // the first failed runtime call
    explicit HostStage(hjr_ctx* c_) : c(c_) {}
    bool ok() const { return rc == HJR_OK && e == hipSuccess; }
    void up(void* dst, const void* src, size_t n) { if (ok() && n) e = hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, c->stream); }
    void down(void* dst, const void* src, size_t n) { if (ok() && n) e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->stream); }
    bool place() // false: the allocation failed, nothing was enqueued and no pointer set
    {
        if (!buf.reserve(total())) return false;
        resolve(buf.p);
        for (const Item& it : items) if (it.src) up((char*)buf.p + it.off, it.src, it.bytes);
        return true;
    }
    void fetch() { for (const Item& it : items) if (it.dst) down(it.dst, (const char*)buf.p + it.off, it.bytes); }
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

// The samples one render call covers: the whole frame, or a sample pass of a progressive frame (include/henjou_hip.h)
struct PassRange {
    bool pass = false;         // a sample pass (else the whole frame, the one-shot launch sequence)
    uint32_t begin = 0, end = 0;
    uint32_t aovs = 0;         // AOVs requested: bit 0 colour, 1 albedo, 2 normal, 3 variance
};
// this rank's share of a frame
struct FrameGeom {
    WorkRect rect; // the window, or else the frame: the extent everything below is derived from
    uint32_t world, tiles_x, chunk_spp, n_chunks;
    uint32_t chunk0, pass_chunks; // the chunks this launch renders: [chunk0, chunk0 + pass_chunks) (all n_chunks for a whole frame)
    uint64_t owned, n_items;
    int lds_mode; // LaunchPlan::lds_mode of the frame data
    PassRange pr;
};

// The functions of hjr_render.hip that hjr_post.hip and hjr_util.hip call
namespace hjr {
bool firefly_keeps_chunks(const hjr_ctx* c);
int check_pass(const hjr_ctx* c, const ParamsW* p, uint32_t aovs, PassRange& r);
int frame_geometry(const hjr_ctx* c, const ParamsW* p, const void* d_color, const PassRange& pr, FrameGeom& g);
void bind_scene_tables(const hjr_ctx* c, KParams& kp);
LaunchPlan plan_launch(const hjr_ctx* c, const KParams& kp, uint64_t n_items, int lds_mode, int integrator, bool fast);
int render_impl(hjr_ctx* c, const ParamsW* p, const PassRange& pr, void* d_color, void* d_albedo, void* d_normal, void* d_var, hipStream_t st, const void* d_prior = nullptr);
} // namespace hjr
#pragma GCC visibility pop
