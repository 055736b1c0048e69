// The utilities of libhenjou_hip.so around a frame: the ray-batch test hook's entry point, the 16-bit stack self-test, tile packing for the
// multi-GPU exchange, the buffers of a bucketed frame, the window blit and the 8-bit preview.
#include "hjr_device_internal.h"
#include "hjr_trace_hook.hip.h"
#include "hjr_image.hip.h"

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
    hjr::bind_scene_tables(c, kp);
    const int lds_mode = launch_layout(c->frame);
    // (`fast` of plan_launch = "megakernel family whatever option pipeline says": the hook has no wavefront path)
    const LaunchPlan pl = hjr::plan_launch(c, kp, n, lds_mode, HJR_INTEGRATOR_NEE, true);
    const size_t rays = (size_t)n * sizeof(hjr_ray);
    TraceArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.round_cap = 2u * n + 64u;
    std::vector<hjr_ray_result> init(n);
    memset(init.data(), 0, rays);
    for (uint32_t i = 0; i < n; i++) { init[i].prim = 0xffffffffu; init[i].status = HJR_TRACE_STATUS_UNTRACED; }
    unsigned long long n_over = 0;
    char* head = nullptr; // 64 zeroed bytes: the pair counter at 0, the overflow counter at 8
    HostStage hs(c);
    hs.add(head, nullptr, nullptr, 64, 16);
    hs.add(a.shadow, shadow, nullptr, rays, 16); hs.add(a.closest, closest, nullptr, rays, 16);
    hs.add(a.out, init.data(), out, rays, 16);
    if (!hs.place()) { set_error("hjr_trace_rays: device allocation failed"); return HJR_ERR_DEVICE; }
    a.next = (unsigned int*)head; a.n_over = (unsigned long long*)(head + 8);
    if (hs.ok()) hs.e = hipMemsetAsync(head, 0, 64, c->stream);
    if (hs.ok()) {
#ifdef HJR_HAVE_FAST
        hs.rc = fast ? hjr_launch_trace_fast(c, pl, loop == HJR_TRACE_FUSED, a, c->stream) : hjr_launch_trace(c, pl, loop == HJR_TRACE_FUSED, a, c->stream);
#else
        hs.rc = hjr_launch_trace(c, pl, loop == HJR_TRACE_FUSED, a, c->stream);
#endif
        if (hs.rc == HJR_OK) hs.e = hipGetLastError();
    }
    hs.fetch();
    hs.down(&n_over, head + 8, 8);
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

// hjr_blit_window_device: a window launch's float4 image into its rectangle of a full-size frame (csrc/hjr_image.hip.h)
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
