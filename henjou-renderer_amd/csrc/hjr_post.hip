// The post stages of libhenjou_hip.so, between a rendered frame and the image a caller gets: filter and spatial variance estimate, G-buffer and coverage pass, temporal accumulation,
// its prior and the context's temporal stage, guided upscale, hjr_render_denoised, assembly of a multi-GPU frame's shards.  Replaces OptixDenoiserManager (renderer/denoiser.h).
#include "hjr_device_internal.h"
#include "hjr_denoise.hip.h"
#include "hjr_temporal.hip.h"
#include "hjr_shards.hip.h"

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
// a host-buffer entry point's staged copy `d` of the frame `f`: M, M^-1 and the G-buffer, with `images` colour and variance, with `history` that
static void stage_side(HostStage& hs, hjr_temporal_frame& d, const hjr_temporal_frame& f, size_t npx, size_t nx, bool images, bool history)
{
    d = f;
    d.color = d.variance = d.history = nullptr;
    hs.add(d.transforms12, f.transforms12, nullptr, nx, 4); hs.add(d.inv_transforms12, f.inv_transforms12, nullptr, nx, 4);
    hs.add(d.gbuffer, f.gbuffer, nullptr, npx * sizeof(hjr_gbuffer_px), 16);
    if (images) { hs.add(d.color, f.color, nullptr, npx * 16, 16); hs.add(d.variance, f.variance, nullptr, npx * 4, 4); }
    if (history) hs.add(d.history, f.history, nullptr, npx * 4, 4);
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
    // One temporary buffer: per side M, M^-1, the G-buffer, colour, variance (prev: history, moments), then the outputs.
    // Alignment: every image starts at a multiple of its element's (16 bytes for float4 and the records, 8 for float2, 4 for float).
    hjr_temporal_frame d[2]; // the staged copies: f[i] with device pointers
    const void* d_prev_mom = nullptr;
    TemporalOut out = {};
    HostStage hs(c);
    for (int i = have_prev ? 0 : 1; i < 2; i++) stage_side(hs, d[i], f[i], npx, nx, true, i == 0);
    if (have_prev && mom) hs.add(d_prev_mom, prev_mom, nullptr, mom, 8);
    hs.add(out.color, nullptr, out_color, npx * 16, 16); hs.add(out.variance, nullptr, out_var, npx * 4, 4); hs.add(out.history, nullptr, out_hist, npx * 4, 4);
    if (mom) hs.add(out.moments, nullptr, out_mom, mom, 8);
    if (resp) hs.add(out.response, nullptr, out_resp, resp, 4);
    if (!hs.place()) { set_error("hjr_temporal_accumulate: device allocation failed"); return HJR_ERR_DEVICE; }
    const TemporalSide ps = have_prev ? temporal_side(d[0], d_prev_mom) : TemporalSide(), cs = temporal_side(d[1], nullptr);
    if (hs.ok()) hs.rc = temporal_launch(c, have_prev ? &ps : nullptr, cs, f[1].width, f[1].height, f[1].n_instances, out, c->stream);
    hs.fetch();
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
    // one temporary buffer: the prior, per side M, M^-1 and the G-buffer (prev: colour, variance, history)
    hjr_temporal_frame d[2];
    void* d_prior = nullptr;
    HostStage hs(c);
    hs.add(d_prior, nullptr, out_prior, npx * 16, 16);
    for (int i = have_prev ? 0 : 1; i < 2; i++) stage_side(hs, d[i], f[i], npx, nx, i == 0, i == 0);
    if (!hs.place()) { set_error("hjr_temporal_prior: device allocation failed"); return HJR_ERR_DEVICE; }
    const TemporalSide ps = have_prev ? temporal_side(d[0], nullptr) : TemporalSide(), cs = temporal_side(d[1], nullptr);
    if (hs.ok()) hs.rc = temporal_prior_launch(c, have_prev ? &ps : nullptr, cs, f[1].width, f[1].height, f[1].n_instances, d_prior, c->stream);
    hs.fetch();
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
    // one temporary buffer: colour, the low-resolution and the output-size records, the output
    const void *d_color, *d_lo, *d_hi; void* d_out;
    HostStage hs(c);
    hs.add(d_color, color_lo, nullptr, n_in * 16, 16); hs.add(d_out, nullptr, out, n_out * 16, 16);
    hs.add(d_lo, gbuffer_lo, nullptr, n_in * sizeof(hjr_gbuffer_px), 16); hs.add(d_hi, gbuffer_hi, nullptr, n_out * sizeof(hjr_gbuffer_px), 16);
    if (!hs.place()) { set_error("hjr_upscale_guided: device allocation failed"); return HJR_ERR_DEVICE; }
    if (hs.ok()) hs.rc = upscale_guided_launch(in_w, in_h, d_color, d_lo, *cam, d_hi, d_out, out_w, out_h, c->stream);
    hs.fetch();
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
        if (const int rc = hjr::check_pass(c, p, (pl.guides ? 7u : 1u) | (pl.with_var ? 8u : 0u), *pr)) return rc;
        if (const int rc = hjr::frame_geometry(c, p, p, *pr, g)) return rc; // (no AOV buffer yet: any non-null pointer)
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
    if (at && hjr::firefly_keeps_chunks(c)) {
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
    if (hs.ok()) hs.rc = hjr::render_impl(c, p, pr, c->d_color.p, pl.guides ? c->d_albedo.p : nullptr, pl.guides ? c->d_normal.p : nullptr, pl.with_var ? c->d_variance.p : nullptr, c->stream, d_prior);
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

// ---- gathered shards of a multi-GPU frame (include/henjou_hip.h; kernel: csrc/hjr_shards.hip.h)
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
