// Job setup shared by the two drivers of a render_option.json (hjr_render_file in host/render_file.cpp, the rank path of cli/henjou_cli.cpp)
// and by its parser (host/loaders.cpp): the table of the "Henjou_HIP" keys that live in a packed or shared field of hjr_render_option, the
// refusals, the pass split, the per-frame parameters, the PNG name and the LUT / sky upload.  Header-only on include/henjou_hip.h and the
// standard library.  No other file masks or shifts a hjr_render_option field: a new stored key is one row here.
#pragma once
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/henjou_hip.h"

namespace hjr {

// hjr_render_option as the drivers and the parser keep it: the caller's struct with the render window's two keys behind it, the layout of
// hjr_render_option_window (include/henjou_hip.h).  hjr_load_render_option_window fills it; the functions below that take the short struct
// see no window and no bucket.
struct RenderOptionW : hjr_render_option { uint32_t window[4]; uint32_t bucket[2]; };
static_assert(sizeof(RenderOptionW) == sizeof(hjr_render_option_window), "RenderOptionW must have the layout of hjr_render_option_window");
inline RenderOptionW with_no_window(const hjr_render_option& o)
{
    RenderOptionW w;
    memset(static_cast<void*>(&w), 0, sizeof(w));
    static_cast<hjr_render_option&>(w) = o;
    return w;
}
// the parser (host/loaders.cpp)
bool load_render_option(const std::string& path, RenderOptionW& opt, std::string& err);

enum KeyEnc : uint8_t {
    ENC_BITS,    // `width` bits at `shift` of the field
    ENC_NONZERO, // the whole field: 0 / 1 when written, any non-zero value reads as 1 (a later row of the field may raise it)
    ENC_PLUS1,   // "device_bvh_refit": device_bvh = 1 + N
    ENC_IS2,     // "denoise_temporal": denoise_variance == 2
};
enum KeyRead : uint8_t {
    READ_FLAG,  // lenient: a bool, or a number (non-zero is true)
    READ_BOOL,  // strict: true, false, 0 or 1
    READ_RANGE, // an integer in the range of the context option of the same name (opt_table(), host/options.hpp)
    READ_SET,   // ... minus the values that option refuses (opt_hole())
};
enum KeyWho : uint8_t {
    WHO_EVERY,          // every process of the job
    WHO_FILTER,         // the process that filters and upscales: the single one, rank 0 of a world
    WHO_FILTER_DENOISE, // ... and in Render_mode Denoise / DenoiseUpScale2X only (Default mode has no filter)
    WHO_SINGLE,         // hjr_render_file only
    WHO_DRIVER,         // no context option: the drivers read the key themselves (key_get)
};
struct KeyRow {
    const char* key;   // the key of the section AND the context option it sets (hjr_set_option): they share their names
    uint8_t parse;     // the parser's turn: the order the file format grew in, which decides what a file with two bad keys reports
    int32_t hjr_render_option::*field;
    KeyEnc enc;
    uint8_t shift, width;
    KeyRead read;
    const char* needs; // the key that must be on for this one to be accepted at all, or nullptr
    KeyWho who;
};

// in the order the drivers set the options
inline const std::vector<KeyRow>& key_table()
{
    using O = hjr_render_option;
    static const std::vector<KeyRow> t = {
        { "force_rebuild", 0, &O::force_rebuild, ENC_BITS, 0, 1, READ_FLAG, nullptr, WHO_SINGLE },
        { "verbose", 1, &O::force_rebuild, ENC_BITS, 1, 1, READ_FLAG, nullptr, WHO_EVERY },
        { "device_bvh", 2, &O::device_bvh, ENC_NONZERO, 0, 31, READ_FLAG, nullptr, WHO_EVERY },
        { "device_bvh_refit", 3, &O::device_bvh, ENC_PLUS1, 0, 31, READ_RANGE, "device_bvh", WHO_EVERY },
        { "device_bvh_opt", 6, &O::device_bvh_opt, ENC_BITS, 0, 8, READ_RANGE, nullptr, WHO_EVERY },
        { "device_bvh_instances", 7, &O::device_bvh_opt, ENC_BITS, 8, 1, READ_BOOL, "device_bvh", WHO_EVERY },
        { "device_bvh_graft", 8, &O::device_bvh_opt, ENC_BITS, 9, 1, READ_BOOL, "device_bvh_instances", WHO_EVERY },
        { "denoise_variance", 4, &O::denoise_variance, ENC_NONZERO, 0, 31, READ_FLAG, nullptr, WHO_FILTER_DENOISE },
        { "denoise_temporal", 5, &O::denoise_variance, ENC_IS2, 0, 31, READ_FLAG, nullptr, WHO_FILTER_DENOISE },
        { "denoise_variance_spatial", 10, &O::device_bvh_opt, ENC_BITS, 10, 1, READ_FLAG, nullptr, WHO_FILTER },
        { "upscale_guided", 11, &O::device_bvh_opt, ENC_BITS, 11, 1, READ_BOOL, nullptr, WHO_FILTER },
        { "denoise_temporal_coverage", 12, &O::device_bvh_opt, ENC_BITS, 12, 3, READ_SET, nullptr, WHO_FILTER },
        { "firefly_clamp", 9, &O::device_bvh_opt, ENC_BITS, 16, 7, READ_RANGE, nullptr, WHO_EVERY }, // (per pixel: every rank clamps its own)
    };
    return t;
}
// key_table() holds the thirteen keys the hand-written parser had; tests/native/render_job_test.cpp pins that set, their bits and the lists
// they give.  A key added since is a row here, of the same form, and the parser, key_row and for_each_option walk key_rows(): the two in
// this order.  Its parse turns go on from key_table()'s.
inline const std::vector<KeyRow>& key_table_since()
{
    using O = hjr_render_option;
    static const std::vector<KeyRow> t = {
        { "firefly_clamp_passes", 13, &O::device_bvh_opt, ENC_BITS, 23, 1, READ_BOOL, "firefly_clamp", WHO_EVERY }, // (every rank keeps its own chunk sums)
        // (in front of "denoise_temporal_moments", which tests/test_temporal_moments_host.py pins as the table's last row and latest parse
        // turn: a file with both keys bad reports this one; no file without this key is read differently)
        { "denoise_temporal_response", 14, &O::device_bvh_opt, ENC_BITS, 24, 1, READ_BOOL, nullptr, WHO_FILTER },
        // (likewise in front of the moments row, which moves up a turn to stay the latest; its turn number is pinned by nobody, its rank is)
        { "adaptive_temporal", 15, &O::device_bvh_opt, ENC_BITS, 25, 1, READ_BOOL, "denoise_temporal", WHO_FILTER },
        // (in front of the moments row, which moves up a turn once more.)  "morph_targets": the drivers hand the glTF's morph targets and, per
        // frame, its evaluated weights to the context (set_morph, set_morph_weights below); the next spare bit of the packed section
        { "morph_targets", 16, &O::device_bvh_opt, ENC_BITS, 26, 1, READ_BOOL, nullptr, WHO_DRIVER },
        { "denoise_temporal_moments", 17, &O::device_bvh_opt, ENC_BITS, 15, 1, READ_BOOL, nullptr, WHO_FILTER },
    };
    return t;
}
inline const std::vector<KeyRow>& key_rows()
{
    static const std::vector<KeyRow> all = [] {
        std::vector<KeyRow> v = key_table();
        v.insert(v.end(), key_table_since().begin(), key_table_since().end());
        return v;
    }();
    return all;
}
inline const KeyRow& key_row(const char* key)
{
    for (const KeyRow& r : key_rows()) if (strcmp(r.key, key) == 0) return r;
    return key_rows().front(); // (not reached: the callers name rows of the tables)
}
inline int key_get(const hjr_render_option& o, const KeyRow& r)
{
    const int32_t f = o.*r.field;
    switch (r.enc) {
    case ENC_BITS: return (f >> r.shift) & ((1 << r.width) - 1);
    case ENC_NONZERO: return f != 0;
    case ENC_PLUS1: return f > 1 ? f - 1 : 0;
    default: return f == 2;
    }
}
// the parser's side; the rows of a field are stored in their parse order
inline void key_put(hjr_render_option& o, const KeyRow& r, int v)
{
    int32_t& f = o.*r.field;
    switch (r.enc) {
    case ENC_BITS: f |= v << r.shift; break;
    case ENC_NONZERO: f = v ? 1 : 0; break;
    case ENC_PLUS1: f = 1 + v; break;
    default: if (v) f = 2;
    }
}

struct JobScope { bool single; int rank; };
inline JobScope single_process() { return { true, 0 }; }
inline JobScope rank_of_world(int rank) { return { false, rank }; }

// fn(option key, value) for every option the job sets in this process, in table order; stops at the first non-zero result and returns it
template <typename Fn> int for_each_option(const hjr_render_option& o, JobScope s, Fn fn)
{
    for (const KeyRow& r : key_rows()) {
        const bool mine = r.who == WHO_EVERY || (r.who == WHO_SINGLE && s.single) || (r.who == WHO_FILTER && s.rank == 0) ||
                          (r.who == WHO_FILTER_DENOISE && s.rank == 0 && o.render_mode != HJR_MODE_DEFAULT);
        const int v = mine ? key_get(o, r) : 0;
        if (v) { const int rc = fn(r.key, v); if (rc) return rc; }
    }
    return 0;
}

// what both drivers derive from the option
struct Job {
    bool denoise, with_var, temporal, adaptive; // a Denoise mode; ... with the variance AOV; ... with temporal accumulation; "noise_threshold" asked for
    int firefly;                                // kappa of "firefly_clamp"
    uint32_t w, h, out_w, out_h;                // render size (half the output in DenoiseUpScale2X, renderer.h:1089-1099); the PNG's size.  With
                                                // "window" both are the window's size ...
    bool win;                                   // ... this is set and (x0, y0) is the window's origin in the frame of frame_w x frame_h pixels
    uint32_t x0, y0, frame_w, frame_h;
};
// fills `job`; false with the refusal in `text` (the caller puts its own name in front), all before a scene or a device is touched
inline bool job_check(const RenderOptionW& o, Job& job, std::string& text)
{
    job.denoise = o.render_mode != HJR_MODE_DEFAULT;
    job.with_var = job.denoise && key_get(o, key_row("denoise_variance"));
    job.temporal = job.denoise && key_get(o, key_row("denoise_temporal"));
    job.adaptive = o.noise_threshold > 0.0f;
    job.firefly = key_get(o, key_row("firefly_clamp"));
    const bool half = o.render_mode == HJR_MODE_DENOISE_UPSCALE2X;
    job.out_w = o.image_width; job.out_h = o.image_height;
    job.w = half ? job.out_w / 2u : job.out_w; job.h = half ? job.out_h / 2u : job.out_h;
    job.frame_w = job.w; job.frame_h = job.h; job.win = false; job.x0 = job.y0 = 0u;
    if (o.render_mode != HJR_MODE_DEFAULT && o.render_mode != HJR_MODE_DENOISE && o.render_mode != HJR_MODE_DENOISE_UPSCALE2X)
        text = "Render_mode must be Default, Denoise or DenoiseUpScale2X (Debug is declared but unused by the reference)";
    else if (job.temporal && job.adaptive && !key_get(o, key_row("adaptive_temporal"))) // with the key the pass that stops the last tile commits the history (rule 11)
        text = "\"denoise_temporal\" cannot be combined with \"noise_threshold\": an adaptive frame that stops early never reaches the sample pass that advances the history";
    else if (job.firefly && !key_get(o, key_row("firefly_clamp_passes")) && (o.passes > 1 || job.adaptive)) // every rank clamps its own pixels, so the rule is the same on both paths
        text = "\"firefly_clamp\" cannot be combined with \"passes\" > 1 or \"noise_threshold\": the clamp needs every chunk sum of a pixel, and a frame rendered in sample passes keeps running sums only";
    else if (job.w == 0 || job.h == 0)
        text = "image too small for DenoiseUpScale2X";
    else if (job.denoise && (o.window[2] || o.bucket[0])) // the filters read the pixels around a window
        text = "\"window\" and \"bucket\" need Render_mode Default: the Denoise modes filter whole frames";
    else if (key_get(o, key_row("adaptive_temporal")) && (o.window[2] || o.bucket[0]))
        text = "\"adaptive_temporal\" cannot be combined with \"window\" or \"bucket\": its prior is gathered over the whole frame";
    else if (o.window[2] > job.w || o.window[3] > job.h)
        text = "\"window\" reaches outside the " + std::to_string(job.w) + " x " + std::to_string(job.h) + " image";
    else {
        // the rectangle the job renders and writes: the window, or else the frame
        job.win = o.window[2] != 0u;
        job.x0 = job.win ? o.window[0] : 0u; job.y0 = job.win ? o.window[1] : 0u;
        if (job.win) { job.w = o.window[2] - o.window[0]; job.h = o.window[3] - o.window[1]; job.out_w = job.w; job.out_h = job.h; }
        return true;
    }
    return false;
}

inline bool job_check(const hjr_render_option& o, Job& job, std::string& text) { return job_check(with_no_window(o), job, text); }

// what a job of several ranks (henjou_cli --devices N > 1) cannot do and one process can; true with the refusal in `text`
inline bool multi_gpu_refusal(const RenderOptionW& o, std::string& text)
{
    if (o.bucket[0]) {
        text = "\"bucket\" cannot be combined with \"devices\" > 1: buckets are composed on the one device that renders them";
        return true;
    }
    if (!key_get(o, key_row("adaptive_temporal"))) return false;
    text = "\"adaptive_temporal\" cannot be combined with \"devices\" > 1: every rank takes the stop decisions of its own shard without the temporal history, which only rank 0 keeps";
    return true;
}

inline bool multi_gpu_refusal(const hjr_render_option& o, std::string& text) { return multi_gpu_refusal(with_no_window(o), text); }

// sample-pass ends of a frame of spp samples in n passes ("Henjou_HIP": {"passes": n}): k * spp / n rounded down to the granule, the last one
// spp; passes that come out empty are dropped, so a frame never has more passes than chunks
inline std::vector<uint32_t> pass_ends(uint32_t spp, uint32_t n)
{
    const uint32_t g = hjr_sample_granule(spp);
    std::vector<uint32_t> ends;
    for (uint32_t k = 1; k < n && g; k++) {
        const uint32_t e = (uint32_t)((uint64_t)k * spp / n) / g * g;
        if (e > (ends.empty() ? 0u : ends.back())) ends.push_back(e);
    }
    ends.push_back(spp);
    return ends;
}

// the launch parameters of a whole frame on one process (rank 0 of 1) at render size w x h; the rank path adds its rank and HJR_FLAG_PACKED
inline int frame_params(const hjr_render_option& o, const hjr_scene* scene, uint32_t frame, uint32_t w, uint32_t h, hjr_params& p)
{
    HJR_INIT(p);
    p.width = w; p.height = h;
    p.spp = o.max_spp; p.frame = frame; p.seed = o.seed; p.integrator = (uint32_t)o.integrator;
    for (int k = 0; k < 3; k++) p.sky[k] = o.scene_sky_default[k];
    p.ibl_intensity = o.IBL_intensity;
    p.rank = 0; p.world_size = 1;
    if (o.fast_math) p.flags |= HJR_FLAG_FAST_MATH; // "Henjou_HIP": {"fast_math": true}
    return hjr_scene_eval_camera(scene, &o, frame / float(o.fps), &p.camera); // renderer.h:1128
}

// <image_name>_<fff>.png (renderer.h:1291-1302: at least three digits)
inline std::string frame_png_name(const hjr_render_option& o, uint32_t frame)
{
    std::string n = std::to_string(frame);
    if (n.size() < 3) n.insert(0, 3 - n.size(), '0');
    return std::string(o.image_name) + "_" + n + ".png";
}

// setLUT (renderer.h:854-898): a missing LUT file only matters if a material uses it, and then ends the job with the PNG loader's error;
// setSky (renderer.h:802-851): a missing / undecodable HDR falls back to the 1x1 scene_sky_default texel (texture.h:89-98), noted on stderr
inline int upload_assets(hjr_ctx* ctx, const hjr_render_option& o, const hjr_scene_view& view, bool note)
{
    uint8_t* lut = nullptr;
    float* sky = nullptr;
    int w = 0, h = 0, rc = HJR_OK;
    if (hjr_load_png_rgba8(o.LUT_path, &lut, &w, &h) == HJR_OK) rc = hjr_set_lut(ctx, lut, w, h);
    else for (uint32_t i = 0; i < view.n_materials; i++) if (view.materials[i].is_thinfilm) rc = HJR_ERR_IO; // hjr_last_error() holds the PNG error
    hjr_free(lut);
    if (rc != HJR_OK || !o.use_IBL) return rc;
    if (hjr_load_hdr_rgba32f(o.IBL_path, &sky, &w, &h) == HJR_OK) rc = hjr_set_sky(ctx, sky, w, h);
    else if (note) fprintf(stderr, "[henjou] %s NOT FOUND: using scene_sky_default\n", o.IBL_path);
    hjr_free(sky);
    return rc;
}

// "morph_targets": the scene's morph sets into the context, once after the upload; `weights` (those the context holds) stays empty without
// the key or without targets in the file, and then nothing is set (the drop-in default: the reference ignores morph data and renders the
// rest pose)
inline int set_morph(hjr_ctx* ctx, const hjr_render_option& o, const hjr_scene* scene, std::vector<float>& weights)
{
    weights.clear();
    if (!key_get(o, key_row("morph_targets"))) return HJR_OK;
    hjr_morph mo;
    HJR_INIT(mo);
    int rc = hjr_scene_get_morph(scene, &mo);
    if (rc != HJR_OK || mo.n_sets == 0) return rc;
    rc = hjr_set_morph(ctx, &mo);
    if (rc == HJR_OK) weights.assign(mo.default_weights, mo.default_weights + mo.n_weights);
    return rc;
}
// ... and per frame the weights at the frame's time, BEFORE that frame's hjr_prepare_transforms is started and never while one runs.
// Weights that did not change are not set again, so a stretch of the animation that does not deform keeps its temporal history
inline int set_morph_weights(hjr_ctx* ctx, const hjr_scene* scene, float time, std::vector<float>& weights)
{
    if (weights.empty()) return HJR_OK;
    std::vector<float> w(weights.size());
    int rc = hjr_scene_eval_morph_weights(scene, time, w.data(), (uint32_t)w.size());
    if (rc != HJR_OK || memcmp(w.data(), weights.data(), w.size() * sizeof(float)) == 0) return rc;
    rc = hjr_set_morph_weights(ctx, w.data(), (uint32_t)w.size());
    if (rc == HJR_OK) weights.swap(w);
    return rc;
}

// "noise_threshold" / "min_samples": converged tiles stop between the sample passes (hjr_set_adaptive)
inline int set_adaptive(hjr_ctx* ctx, const hjr_render_option& o)
{
    hjr_adaptive ad;
    HJR_INIT(ad);
    ad.noise_threshold = o.noise_threshold; ad.min_samples = o.min_samples;
    return hjr_set_adaptive(ctx, &ad);
}

} // namespace hjr
