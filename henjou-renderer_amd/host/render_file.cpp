// The whole-file driver of the C-ABI: hjr_render_file == Renderer::initializeAndRender (renderer/renderer.h:1053-1317).  The one host
// file that drives the device half of the library (context, uploads, sample passes, adaptive sampling) through its public entry points.
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

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
    hjr_scene* scene = nullptr;
    rc = hjr_scene_load_gltf(opt.gltf_path, opt.gltf_name, &opt, &scene);
    if (rc != HJR_OK) return rc;
    hjr_ctx* ctx = nullptr;
    rc = hjr_create(device, &ctx);
    if (rc != HJR_OK) { hjr_scene_free(scene); return rc; }
    hjr_scene_view view;
    HJR_INIT(view);
    hjr_scene_get_view(scene, &view);
    rc = hjr::for_each_option(opt, hjr::single_process(), [&](const char* key, int value) { return hjr_set_option(ctx, key, value); });
    const bool adaptive = job.adaptive; // "noise_threshold": converged tiles stop between the sample passes
    if (rc == HJR_OK) rc = hjr_upload_scene(ctx, &view);
    if (rc == HJR_OK && adaptive) rc = hjr::set_adaptive(ctx, opt);
    if (rc == HJR_OK) rc = hjr::upload_assets(ctx, opt, view, true);
    std::vector<float> morph_w; // "morph_targets": the glTF's morph sets, once; the weights per frame below
    if (rc == HJR_OK) rc = hjr::set_morph(ctx, opt, scene, morph_w);
    std::vector<float> m((size_t)view.n_instances * 12), inv((size_t)view.n_instances * 12);
    const size_t npx = (size_t)job.out_w * job.out_h; // (the window's size with "window")
    // Output stage off the critical path: float4 -> sRGB8 -> PNG -> file runs on a writer thread while the main thread
    // already builds and renders the next frame (two frame buffers in rotation).  The reference's loop is serial
    // (renderer.h:1281-1302); the files are the same.  Only aov_color is produced: Default mode never reads the albedo /
    // normal AOVs (they feed the OptiX denoiser, denoiser.h:94-97).  "Henjou_HIP": {"serial_io": true} disables the overlap.
    struct Slot { std::vector<float> color; std::string name; bool full = false; };
    Slot slots[2];
    for (Slot& sl : slots) sl.color.resize(npx * 4);
    std::mutex mu;
    std::condition_variable cv;
    bool quit = false;
    int write_rc = HJR_OK;
    std::string write_err;
    const bool serial_io = opt.serial_io != 0;
    auto write_slot = [&](Slot& sl) -> int {
        std::vector<uint8_t> rgba8(npx * 4);
        hjr::float4_to_srgb8(sl.color.data(), rgba8.data(), (uint32_t)npx);
        std::string err;
        if (!hjr::write_png(sl.name, rgba8.data(), job.out_w, job.out_h, true, err)) {
            std::lock_guard<std::mutex> lk(mu);
            write_err = err;
            return HJR_ERR_IO;
        }
        return HJR_OK;
    };
    std::thread writer;
    if (!serial_io)
        writer = std::thread([&]() {
            int next = 0;
            for (;;) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return slots[next].full || quit; });
                    if (!slots[next].full) return; // quit with nothing pending
                }
                const int r = write_slot(slots[next]);
                {
                    std::lock_guard<std::mutex> lk(mu);
                    slots[next].full = false;
                    if (r != HJR_OK && write_rc == HJR_OK) write_rc = r;
                }
                cv.notify_all();
                next ^= 1;
            }
        });
    int cur = 0;
    const auto t_all0 = std::chrono::steady_clock::now();
    uint32_t n_frames = 0;
    // scene update of frame f + 1 (host: TRS evaluation, flatten, BVH build) runs on a helper thread while frame f renders;
    // only its upload (hjr_commit_transforms) waits for the render.  The reference's loop is serial (renderer.h:1128-1137).
    std::thread prep;
    int prep_rc = HJR_OK;
    std::string prep_err;
    auto prepare = [&](uint32_t frame) {
        float time = frame / float(opt.fps); // renderer.h:1128
        hjr_scene_eval_transforms(scene, time, m.data(), inv.data());
        prep_rc = hjr_prepare_transforms(ctx, m.data(), inv.data(), view.n_instances);
        if (prep_rc != HJR_OK) prep_err = hjr_last_error(); // thread-local on the helper thread
    };
    // "morph_targets": the weights of a frame are set on this thread before its prepare is started (and the previous one has been joined):
    // hjr_set_morph_weights must not run concurrently with hjr_prepare_transforms.  It ends no frame: frame f has not begun its passes
    auto weights = [&](uint32_t frame) { return hjr::set_morph_weights(ctx, scene, frame / float(opt.fps), morph_w); };
    if (rc == HJR_OK && opt.start_frame < opt.end_frame) rc = weights(opt.start_frame);
    if (rc == HJR_OK && opt.start_frame < opt.end_frame) prepare(opt.start_frame);
    for (uint32_t frame = opt.start_frame; rc == HJR_OK && frame < opt.end_frame; frame++) {
        if (prep.joinable()) prep.join();
        if (prep_rc != HJR_OK) { rc = prep_rc; set_error(prep_err); break; }
        rc = hjr_commit_transforms(ctx);
        if (rc != HJR_OK) break;
        if (frame + 1 < opt.end_frame && !serial_io) {
            rc = weights(frame + 1);
            if (rc != HJR_OK) break;
            prep = std::thread(prepare, frame + 1);
        }
        hjr_params_window pw; // (the longer caller: the render window behind hjr_params)
        memset(&pw, 0, sizeof(pw));
        hjr_params& p = pw.p;
        rc = hjr::frame_params(opt, scene, frame, job.frame_w, job.frame_h, p);
        if (rc != HJR_OK) break;
        p.struct_size = (uint32_t)sizeof(pw);
        if (job.win) memcpy(pw.window, opt.window, sizeof(pw.window)); // "window": every launch of the frame renders that rectangle
        Slot& sl = slots[cur];
        if (!serial_io) { // the slot may still be with the writer (two frames behind)
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !sl.full; });
            if (write_rc != HJR_OK) { rc = write_rc; break; }
        }
        // "passes": the frame in sample passes; each pass overwrites the slot with the running mean, the last one with the frame
        const std::vector<uint32_t> ends = hjr::pass_ends(p.spp, opt.passes ? opt.passes : 1u);
        // "noise_threshold": the frame ends with the first pass that leaves no tile active; the slot then holds the frame
        float kernel_ms = 0.0f;
        size_t n_done = 0;
        hjr_adaptive_state as;
        HJR_INIT(as);
        // "bucket": the frame (the window, when there is one) bucket by bucket.  A bucket goes through all its sample passes, adaptive stop
        // included, into a bucket-sized device buffer and is then written into the frame on the device; the frame comes down once.  Every
        // buffer the context keeps for a launch (chunk sums, running sums, adaptive state) has the bucket's size.
        const uint32_t n_buckets = opt.bucket[0] ? hjr_bucket_count(job.w, job.h, opt.bucket[0], opt.bucket[1]) : 0u;
        void *d_frame = nullptr, *d_bucket = nullptr;
        if (n_buckets) rc = hjr::bucket_buffer(ctx, 0, npx * 16, &d_frame);
        for (uint32_t b = 0; rc == HJR_OK && b < n_buckets; b++) {
            uint32_t rel[4]; // the bucket inside the job's rectangle; + its origin: the launch's window
            rc = hjr_bucket_window(job.w, job.h, opt.bucket[0], opt.bucket[1], b, rel);
            if (rc != HJR_OK) break;
            hjr_params_window pb = pw;
            pb.window[0] = job.x0 + rel[0]; pb.window[1] = job.y0 + rel[1]; pb.window[2] = job.x0 + rel[2]; pb.window[3] = job.y0 + rel[3];
            rc = hjr::bucket_buffer(ctx, 1, (size_t)(rel[2] - rel[0]) * (rel[3] - rel[1]) * 16, &d_bucket);
            for (size_t k = 0; rc == HJR_OK && k < ends.size(); k++) {
                if (ends.size() > 1) { pb.p.sample_begin = k ? ends[k - 1] : 0u; pb.p.sample_end = ends[k]; }
                rc = hjr_render_device(ctx, &pb.p, d_bucket, nullptr, nullptr, nullptr);
                if (rc != HJR_OK) break;
                hjr_stats st;
                HJR_INIT(st);
                if (hjr_get_stats(ctx, &st) == HJR_OK) kernel_ms += st.last_kernel_ms;
                if (k + 1 > n_done) n_done = k + 1; // (the note: the most passes any bucket of the frame took)
                if (rc == HJR_OK && adaptive && ends.size() > 1) {
                    hjr_adaptive_state ab;
                    HJR_INIT(ab);
                    rc = hjr_get_adaptive_state(ctx, &ab);
                    if (rc != HJR_OK) break;
                    const bool over = ab.active_tiles == 0 || k + 1 == ends.size();
                    if (over) { as.owned_tiles += ab.owned_tiles; as.active_tiles += ab.active_tiles; as.samples_rendered += ab.samples_rendered; if (ab.sample_end > as.sample_end) as.sample_end = ab.sample_end; } // (tiles and samples of all buckets; the latest pass end of any)
                    if (ab.active_tiles == 0) break;
                }
            }
            if (rc == HJR_OK) rc = hjr_blit_window_device(ctx, d_bucket, rel, d_frame, job.w, job.h, nullptr);
        }
        if (rc == HJR_OK && n_buckets) rc = hjr::bucket_download(ctx, sl.color.data(), d_frame, npx * 16);
        for (size_t k = 0; rc == HJR_OK && !n_buckets && k < ends.size(); k++) {
            if (ends.size() > 1) { p.sample_begin = k ? ends[k - 1] : 0u; p.sample_end = ends[k]; }
            if (opt.render_mode == HJR_MODE_DEFAULT) rc = hjr_render(ctx, &p, sl.color.data(), nullptr, nullptr);
            else rc = hjr_render_denoised(ctx, &p, opt.render_mode, sl.color.data(), opt.image_width, opt.image_height); // renderer.h:1258-1281
            hjr_stats st;
            HJR_INIT(st);
            if (rc == HJR_OK && hjr_get_stats(ctx, &st) == HJR_OK) kernel_ms += st.last_kernel_ms;
            n_done++;
            if (rc == HJR_OK && adaptive && ends.size() > 1) {
                rc = hjr_get_adaptive_state(ctx, &as);
                if (rc == HJR_OK && as.active_tiles == 0) break;
            }
        }
        if (rc != HJR_OK) break;
        std::string note = ends.size() > 1 ? ", " + std::to_string(n_done) + " sample passes" + (n_buckets ? " at most per bucket" : "") : "";
        if (adaptive && ends.size() > 1)
            note += ", adaptive: " + std::to_string(as.active_tiles) + " of " + std::to_string(as.owned_tiles) + " tiles active at " + std::to_string(as.sample_end) + " spp, " +
                    std::to_string(as.samples_rendered) + " samples rendered";
        if (n_buckets) note += ", " + std::to_string(n_buckets) + " buckets";
        fprintf(stderr, "[henjou] frame %u: %ux%u, %u spp, kernel %.3f ms (%.2f Msamples/s)%s\n", frame, job.w, job.h, p.spp,
                kernel_ms, kernel_ms > 0 ? (double)job.w * job.h * p.spp / (kernel_ms * 1e3) : 0.0, note.c_str());
        sl.name = hjr::frame_png_name(opt, frame);
        n_frames++;
        if (serial_io) { rc = write_slot(sl); if (rc != HJR_OK) set_error(write_err); if (rc == HJR_OK && frame + 1 < opt.end_frame) rc = weights(frame + 1); if (rc == HJR_OK && frame + 1 < opt.end_frame) prepare(frame + 1); }
        else {
            { std::lock_guard<std::mutex> lk(mu); sl.full = true; }
            cv.notify_all();
            cur ^= 1;
        }
    }
    if (prep.joinable()) prep.join();
    if (!serial_io) {
        { // drain: the writer takes the slots in order, then quits
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !slots[0].full && !slots[1].full; });
            quit = true;
        }
        cv.notify_all();
        writer.join();
        if (rc == HJR_OK && write_rc != HJR_OK) { rc = write_rc; set_error(write_err); }
    }
    if (n_frames) {
        const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_all0).count();
        fprintf(stderr, "[henjou] %u frame(s) in %.3f s wall (%.1f ms per frame incl. scene update, download and PNG output)\n", n_frames, wall, 1e3 * wall / n_frames);
    }
    hjr_destroy(ctx);
    hjr_scene_free(scene);
    return rc;
}
