// The whole-file driver of the C-ABI: hjr_render_file == Renderer::initializeAndRender (renderer/renderer.h:1053-1317).  The one host
// file that drives the device half of the library (context, uploads, sample passes, adaptive sampling) through its public entry points.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "frame_loop.hpp"
#include "render_job.hpp"

namespace hjr {
void set_error(const std::string& s);
bool write_png(const std::string& path, const uint8_t* rgba, uint32_t w, uint32_t h, bool flip_y, std::string& err);
void float4_to_srgb8(const float* rgba, uint8_t* out, uint32_t n);
// "bucket" (csrc/hjr_util.hip): two buffers of the context for a bucketed frame, slot 0 the frame and slot 1 a bucket, and the frame's one
// download on the context's stream (synchronous)
int bucket_buffer(hjr_ctx* c, int slot, size_t bytes, void** d_out);
int bucket_download(hjr_ctx* c, float* host, const void* d_frame, size_t bytes);
} // namespace hjr
using hjr::set_error;

namespace {

// scene and context of a job, released on every return path.  Declared in front of the writer and the scene update, so both threads have
// been joined when the context goes
struct JobGuard {
    hjr_scene* scene = nullptr;
    hjr_ctx* ctx = nullptr;
    ~JobGuard() { if (ctx) hjr_destroy(ctx); if (scene) hjr_scene_free(scene); }
};

// what the sample passes of a frame came to, for its line on stderr
struct FrameTally {
    float kernel_ms = 0.0f;
    uint32_t buckets = 0;  // 0: the frame was not bucketed
    uint32_t passes = 0;   // (bucketed: the most any bucket took)
    hjr_adaptive_state as; // (bucketed: tiles and samples of all buckets; the latest pass end of any)
};

// One frame into `color` (job.out_w x job.out_h float4).  "passes": the frame in sample passes (render_passes, frame_loop.hpp); each pass
// overwrites `color` with the running mean, the last one with the frame.  "noise_threshold": the frame ends with the first pass that leaves
// no tile active; `color` then holds the frame.
// "bucket": the frame (the window, when there is one) bucket by bucket.  A bucket goes through all its sample passes, adaptive stop
// included, into a bucket-sized device buffer and is then written into the frame on the device; the frame comes down once.  Every
// buffer the context keeps for a launch (chunk sums, running sums, adaptive state) has the bucket's size.
int render_frame(hjr_ctx* ctx, const hjr::RenderOptionW& opt, const hjr::Job& job, const hjr_params_window& pw, const std::vector<uint32_t>& ends, float* color, FrameTally& t)
{
    const bool split = opt.passes > 1;
    auto add_kernel_ms = [&](uint32_t) { // (hjr_get_stats waits for the pass)
        hjr_stats st;
        HJR_INIT(st);
        if (hjr_get_stats(ctx, &st) == HJR_OK) t.kernel_ms += st.last_kernel_ms;
        return HJR_OK;
    };
    std::function<int(hjr_adaptive_state&)> adaptive_state;
    if (job.adaptive) adaptive_state = [ctx](hjr_adaptive_state& s) { return hjr_get_adaptive_state(ctx, &s); };
    HJR_INIT(t.as);
    const uint32_t n_buckets = t.buckets = opt.bucket[0] ? hjr_bucket_count(job.w, job.h, opt.bucket[0], opt.bucket[1]) : 0u;
    if (!n_buckets) {
        hjr_params_window pf = pw;
        const hjr::PassRun run = hjr::render_passes(ends, pf.p, split, [&](hjr_params& p) {
            if (opt.render_mode == HJR_MODE_DEFAULT) return hjr_render(ctx, &p, color, nullptr, nullptr);
            return hjr_render_denoised(ctx, &p, opt.render_mode, color, opt.image_width, opt.image_height); // renderer.h:1258-1281
        }, add_kernel_ms, adaptive_state);
        t.passes = run.done;
        if (run.queried) t.as = run.state;
        return run.rc;
    }
    const size_t npx = (size_t)job.out_w * job.out_h;
    void *d_frame = nullptr, *d_bucket = nullptr;
    int rc = hjr::bucket_buffer(ctx, 0, npx * 16, &d_frame);
    for (uint32_t b = 0; rc == HJR_OK && b < n_buckets; b++) {
        uint32_t rel[4]; // the bucket inside the job's rectangle; + its origin: the launch's window
        rc = hjr_bucket_window(job.w, job.h, opt.bucket[0], opt.bucket[1], b, rel);
        if (rc != HJR_OK) break;
        hjr_params_window pb = pw;
        pb.window[0] = job.x0 + rel[0]; pb.window[1] = job.y0 + rel[1]; pb.window[2] = job.x0 + rel[2]; pb.window[3] = job.y0 + rel[3];
        rc = hjr::bucket_buffer(ctx, 1, (size_t)(rel[2] - rel[0]) * (rel[3] - rel[1]) * 16, &d_bucket);
        if (rc != HJR_OK) break;
        const hjr::PassRun run = hjr::render_passes(ends, pb.p, split, [&](hjr_params& p) { return hjr_render_device(ctx, &p, d_bucket, nullptr, nullptr, nullptr); },
                                                    add_kernel_ms, adaptive_state);
        if (run.done > t.passes) t.passes = run.done;
        if ((rc = run.rc) != HJR_OK) break;
        if (run.queried) {
            t.as.owned_tiles += run.state.owned_tiles; t.as.active_tiles += run.state.active_tiles; t.as.samples_rendered += run.state.samples_rendered;
            if (run.state.sample_end > t.as.sample_end) t.as.sample_end = run.state.sample_end;
        }
        rc = hjr_blit_window_device(ctx, d_bucket, rel, d_frame, job.w, job.h, nullptr);
    }
    if (rc == HJR_OK) rc = hjr::bucket_download(ctx, color, d_frame, npx * 16);
    return rc;
}

void print_frame_note(const hjr::Job& job, uint32_t frame, uint32_t spp, bool several, const FrameTally& t)
{
    const uint32_t n_buckets = t.buckets;
    std::string note = several ? ", " + std::to_string(t.passes) + " sample passes" + (n_buckets ? " at most per bucket" : "") : "";
    if (job.adaptive && several)
        note += ", adaptive: " + std::to_string(t.as.active_tiles) + " of " + std::to_string(t.as.owned_tiles) + " tiles active at " + std::to_string(t.as.sample_end) + " spp, " +
                std::to_string(t.as.samples_rendered) + " samples rendered";
    if (n_buckets) note += ", " + std::to_string(n_buckets) + " buckets";
    fprintf(stderr, "[henjou] frame %u: %ux%u, %u spp, kernel %.3f ms (%.2f Msamples/s)%s\n", frame, job.w, job.h, spp, t.kernel_ms,
            t.kernel_ms > 0 ? (double)job.w * job.h * spp / (t.kernel_ms * 1e3) : 0.0, note.c_str());
}

} // namespace

// Renderer::initializeAndRender — renderer/renderer.h:1053-1317.  Render_mode "Default" is the pass-through of the reference
// (its denoiser runs with blendFactor 1); "Denoise" / "DenoiseUpScale2X" keep the reference's data flow with the HIP a-trous
// filter in place of the closed OptiX network (csrc/hjr_denoise.hip.h).
extern "C" int hjr_render_file(const char* render_option_json, int device)
{
    if (!render_option_json) { set_error("hjr_render_file: null path"); return HJR_ERR_ARG; }
    hjr::RenderOptionW opt; // (the long form: "window" and "bucket" behind hjr_render_option)
    memset(static_cast<void*>(&opt), 0, sizeof(opt));
    opt.struct_size = (uint32_t)sizeof(opt);
    int rc = hjr_load_render_option_window(render_option_json, &opt);
    if (rc != HJR_OK) return rc;
    hjr::Job job; // the refusals come before the scene and the device (host/render_job.hpp)
    std::string refusal;
    if (!hjr::job_check(opt, job, refusal)) { set_error("hjr_render_file: " + refusal); return HJR_ERR_ARG; }
    JobGuard g;
    rc = hjr_scene_load_gltf(opt.gltf_path, opt.gltf_name, &opt, &g.scene);
    if (rc == HJR_OK) rc = hjr_create(device, &g.ctx);
    if (rc != HJR_OK) return rc;
    hjr_scene* const scene = g.scene;
    hjr_ctx* const ctx = g.ctx;
    hjr_scene_view view;
    HJR_INIT(view);
    hjr_scene_get_view(scene, &view);
    rc = hjr::for_each_option(opt, hjr::single_process(), [&](const char* key, int value) { return hjr_set_option(ctx, key, value); });
    if (rc == HJR_OK) rc = hjr_upload_scene(ctx, &view);
    if (rc == HJR_OK && job.adaptive) rc = hjr::set_adaptive(ctx, opt); // "noise_threshold": converged tiles stop between the sample passes
    if (rc == HJR_OK) rc = hjr::upload_assets(ctx, opt, view, true);
    std::vector<float> morph_w; // "morph_targets": the glTF's morph sets, once; the weights per frame below
    if (rc == HJR_OK) rc = hjr::set_morph(ctx, opt, scene, morph_w);
    if (rc != HJR_OK) return rc;
    const size_t npx = (size_t)job.out_w * job.out_h; // (the window's size with "window")
    const bool serial_io = opt.serial_io != 0;
    // Output stage off the critical path: float4 -> sRGB8 -> PNG -> file runs on a writer thread while this thread already builds and
    // renders the next frame.  The reference's loop is serial (renderer.h:1281-1302); the files are the same.  Only aov_color is
    // produced: Default mode never reads the albedo / normal AOVs (they feed the OptiX denoiser, denoiser.h:94-97).
    // "Henjou_HIP": {"serial_io": true} disables the overlap, here and below.
    hjr::FrameWriter writer(npx * 4, [&](const float* rgba, const std::string& name, std::string& err) {
        std::vector<uint8_t> rgba8(npx * 4);
        hjr::float4_to_srgb8(rgba, rgba8.data(), (uint32_t)npx);
        return hjr::write_png(name, rgba8.data(), job.out_w, job.out_h, true, err) ? HJR_OK : HJR_ERR_IO;
    }, serial_io);
    // scene update of frame f + 1 (host: TRS evaluation, flatten, BVH build) runs on a helper thread while frame f renders; only its
    // upload (hjr_commit_transforms) waits for the render.  The reference's loop is serial (renderer.h:1128-1137).
    std::vector<float> m((size_t)view.n_instances * 12), inv((size_t)view.n_instances * 12);
    hjr::ScenePrefetch update([&](uint32_t frame) {
        hjr_scene_eval_transforms(scene, frame / float(opt.fps), m.data(), inv.data()); // renderer.h:1128
        return hjr_prepare_transforms(ctx, m.data(), inv.data(), view.n_instances);
    }, [] { return std::string(hjr_last_error()); }, serial_io);
    // "morph_targets": the weights of a frame are set on this thread, between take() and start() (ScenePrefetch's rule).  It ends no
    // frame: frame f has not begun its passes
    auto start_update = [&](uint32_t frame) {
        if (frame >= opt.end_frame) return HJR_OK;
        const int r = hjr::set_morph_weights(ctx, scene, frame / float(opt.fps), morph_w);
        return r != HJR_OK ? r : update.start(frame);
    };
    const auto t_all0 = std::chrono::steady_clock::now();
    uint32_t n_frames = 0;
    std::string err;
    auto failed = [&](int r) { if (r != HJR_OK) set_error(err); return r != HJR_OK; }; // (a result that came with its text in `err`)
    rc = start_update(opt.start_frame);
    for (uint32_t frame = opt.start_frame; rc == HJR_OK && frame < opt.end_frame; frame++) {
        if (failed(rc = update.take(err))) break;
        rc = hjr_commit_transforms(ctx);
        if (rc == HJR_OK && !serial_io) rc = start_update(frame + 1);
        if (rc != HJR_OK) break;
        hjr_params_window pw; // (the longer caller: the render window behind hjr_params)
        memset(&pw, 0, sizeof(pw));
        rc = hjr::frame_params(opt, scene, frame, job.frame_w, job.frame_h, pw.p);
        if (rc != HJR_OK) break;
        pw.p.struct_size = (uint32_t)sizeof(pw);
        if (job.win) memcpy(pw.window, opt.window, sizeof(pw.window)); // "window": every launch of the frame renders that rectangle
        float* color = nullptr;
        if (failed(rc = writer.acquire(color, err))) break;
        const std::vector<uint32_t> ends = hjr::pass_ends(pw.p.spp, opt.passes ? opt.passes : 1u);
        FrameTally tally;
        rc = render_frame(ctx, opt, job, pw, ends, color, tally);
        if (rc != HJR_OK) break;
        print_frame_note(job, frame, pw.p.spp, ends.size() > 1, tally);
        n_frames++;
        if (failed(rc = writer.submit(hjr::frame_png_name(opt, frame), err))) break;
        if (serial_io) rc = start_update(frame + 1);
    }
    const int write_rc = writer.drain(err);
    if (rc == HJR_OK) failed(rc = write_rc);
    if (n_frames) {
        const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_all0).count();
        fprintf(stderr, "[henjou] %u frame(s) in %.3f s wall (%.1f ms per frame incl. scene update, download and PNG output)\n", n_frames, wall, 1e3 * wall / n_frames);
    }
    return rc;
}
