// Host half of the C-ABI (include/henjou_hip.h): scene surface and output stage (the whole-file driver hjr_render_file is
// host/render_file.cpp).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/henjou_hip.h"
#include "../csrc/hjr_layout.h"
#include "abi.hpp"
#include "scene.hpp"
#include "render_job.hpp"

namespace hjr {
static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }
bool write_png(const std::string& path, const uint8_t* rgba, uint32_t w, uint32_t h, bool flip_y, std::string& err);
bool read_png_rgba8(const std::string& path, std::vector<uint8_t>& rgba, int& w, int& h, std::string& err);
bool read_image_rgba8(const std::string& path, std::vector<uint8_t>& rgba, int& w, int& h, std::string& err);
bool write_pfm(const std::string& path, const float* rgba, uint32_t w, uint32_t h, std::string& err);
bool read_hdr_rgba32f(const std::string& path, std::vector<float>& rgba, int& w, int& h, std::string& err);
void float4_to_srgb8(const float* rgba, uint8_t* out, uint32_t n);
void tonemap_to_srgb8(const float* rgba, uint8_t* out, uint32_t n, int mode);
} // namespace hjr
using hjr::set_error;

struct hjr_scene {
    hjr::SceneData data;
};

extern "C" const char* hjr_last_error(void) { return hjr::g_err.c_str(); }

extern "C" int hjr_load_render_option(const char* json_path, hjr_render_option* out)
{
    if (!json_path || !out) { set_error("hjr_load_render_option: null argument"); return HJR_ERR_ARG; }
    uint32_t out_size;
    if (!hjr::abi_size(out, out_size, "hjr_load_render_option")) return HJR_ERR_ARG;
    std::string err;
    hjr_render_option opt;
    if (!hjr::load_render_option(json_path, opt, err)) {
        set_error(err);
        return err.rfind("File ", 0) == 0 ? HJR_ERR_IO : HJR_ERR_PARSE;
    }
    opt.struct_size = (uint32_t)sizeof(opt);
    return hjr::abi_give(out, opt, "hjr_load_render_option") ? HJR_OK : HJR_ERR_ARG; // sized struct: at most out->struct_size bytes are written
}
// the same for a caller with hjr_render_option_window (or any shorter struct): the keys "window" and "bucket" are handed out too
extern "C" int hjr_load_render_option_window(const char* json_path, hjr_render_option* out)
{
    if (!json_path || !out) { set_error("hjr_load_render_option_window: null argument"); return HJR_ERR_ARG; }
    uint32_t n;
    if (!hjr::abi_size(out, n, "hjr_load_render_option_window")) return HJR_ERR_ARG;
    std::string err;
    hjr::RenderOptionW opt;
    if (!hjr::load_render_option(json_path, opt, err)) {
        set_error(err);
        return err.rfind("File ", 0) == 0 ? HJR_ERR_IO : HJR_ERR_PARSE;
    }
    opt.struct_size = n; // (abi_give for the long struct: the caller's struct_size stays what it was)
    memcpy(static_cast<void*>(out), &opt, std::min<size_t>(n, sizeof(opt)));
    return HJR_OK;
}

extern "C" int hjr_scene_load_gltf(const char* dir, const char* file, hjr_render_option* opt, hjr_scene** out)
{
    if (!dir || !file || !opt || !out) { set_error("hjr_scene_load_gltf: null argument"); return HJR_ERR_ARG; }
    *out = nullptr;
    hjr_render_option o; // sized struct, in / out: the loader may enable the camera animation (gltfloader.h:1296-1310)
    if (!hjr::abi_take(opt, o, "hjr_scene_load_gltf")) return HJR_ERR_ARG;
    const std::string dir_s = dir, file_s = file; // (dir / file usually point into *opt)
    hjr_scene* s = new hjr_scene();
    std::string err;
    if (!hjr::load_gltf(dir_s, file_s, s->data, o, err)) {
        set_error(err);
        delete s;
        return err.find("cannot open") != std::string::npos ? HJR_ERR_IO : HJR_ERR_PARSE;
    }
    if (!hjr::abi_give(opt, o, "hjr_scene_load_gltf")) { delete s; return HJR_ERR_ARG; }
    *out = s;
    return HJR_OK;
}

extern "C" void hjr_scene_free(hjr_scene* s) { delete s; }

extern "C" int hjr_scene_get_view(const hjr_scene* s, hjr_scene_view* v)
{
    if (!s || !v) { set_error("hjr_scene_get_view: null argument"); return HJR_ERR_ARG; }
    hjr_scene_view* const user = v;
    hjr_scene_view full; // sized struct: filled here, at most user->struct_size bytes handed out
    v = &full;
    const hjr::SceneData& d = s->data;
    memset(v, 0, sizeof(*v));
    v->struct_size = (uint32_t)sizeof(*v);
    v->n_vertices = (uint32_t)d.vertices.size();
    v->n_triangles = (uint32_t)(d.indices.size() / 3);
    v->n_instances = (uint32_t)d.instances.size();
    v->n_materials = (uint32_t)d.materials.size();
    v->n_lights = (uint32_t)d.light_prim_ids.size();
    v->n_animations = (uint32_t)d.animations.size();
    v->vertices = d.vertices.empty() ? nullptr : &d.vertices[0].x;
    v->normals = d.normals.empty() ? nullptr : &d.normals[0].x;
    v->texcoords = d.texcoords.empty() ? nullptr : &d.texcoords[0].x;
    v->indices = d.indices.data();
    v->material_ids = d.material_ids.data();
    v->prim_offset = d.prim_offset.data();
    v->geometry_index_offset = d.geo_index_offset.data();
    v->geometry_index_count = d.geo_index_count.data();
    v->instance_animation_id = d.inst_animation_id.data();
    v->materials = d.materials.data();
    v->light_prim_ids = d.light_prim_ids.data();
    v->light_prim_emission = d.light_prim_emission.empty() ? nullptr : &d.light_prim_emission[0].x;
    v->n_textures = (uint32_t)d.texture_views.size();
    v->textures = d.texture_views.data();
    return hjr::abi_give(user, full, "hjr_scene_get_view") ? HJR_OK : HJR_ERR_ARG;
}

extern "C" int hjr_scene_get_morph(const hjr_scene* s, hjr_morph* out)
{
    if (!s || !out) { set_error("hjr_scene_get_morph: null argument"); return HJR_ERR_ARG; }
    const hjr::SceneData& d = s->data;
    hjr_morph full; // sized struct: borrowed pointers, valid as long as the scene; n_sets == 0: the file has no morph targets
    memset(&full, 0, sizeof(full));
    full.struct_size = (uint32_t)sizeof(full);
    full.n_sets = (uint32_t)d.morph_views.size();
    full.n_weights = (uint32_t)d.morph_default_weights.size();
    full.sets = d.morph_views.empty() ? nullptr : d.morph_views.data();
    full.default_weights = d.morph_default_weights.empty() ? nullptr : d.morph_default_weights.data();
    return hjr::abi_give(out, full, "hjr_scene_get_morph") ? HJR_OK : HJR_ERR_ARG;
}

extern "C" int hjr_scene_eval_morph_weights(const hjr_scene* s, float time, float* w, uint32_t n)
{
    if (!s || (n && !w)) { set_error("hjr_scene_eval_morph_weights: null argument"); return HJR_ERR_ARG; }
    if (n != s->data.morph_default_weights.size()) { set_error("hjr_scene_eval_morph_weights: weight count does not match the scene's n_weights"); return HJR_ERR_ARG; }
    hjr::eval_morph_weights(s->data, time, w);
    return HJR_OK;
}

extern "C" int hjr_scene_eval_transforms(const hjr_scene* s, float time, float* m12, float* inv12)
{
    if (!s || ((!m12 || !inv12) && !s->data.instances.empty())) { set_error("hjr_scene_eval_transforms: null argument"); return HJR_ERR_ARG; }
    hjr::eval_transforms(s->data, time, m12, inv12);
    return HJR_OK;
}

extern "C" int hjr_scene_eval_camera(const hjr_scene* s, const hjr_render_option* opt, float time, hjr_camera* out)
{
    if (!s || !opt || !out) { set_error("hjr_scene_eval_camera: null argument"); return HJR_ERR_ARG; }
    hjr_render_option o; // sized struct
    if (!hjr::abi_take(opt, o, "hjr_scene_eval_camera")) return HJR_ERR_ARG;
    hjr::eval_camera(s->data, o, time, *out);
    return HJR_OK;
}

extern "C" int hjr_load_png_rgba8(const char* path, uint8_t** rgba, int* w, int* h)
{
    if (!path || !rgba || !w || !h) { set_error("hjr_load_png_rgba8: null argument"); return HJR_ERR_ARG; }
    std::vector<uint8_t> px;
    std::string err;
    if (!hjr::read_png_rgba8(path, px, *w, *h, err)) {
        set_error(err);
        return err.rfind("cannot open", 0) == 0 ? HJR_ERR_IO : HJR_ERR_PARSE;
    }
    *rgba = (uint8_t*)malloc(px.size());
    if (!*rgba) { set_error("out of memory"); return HJR_ERR_ARG; }
    memcpy(*rgba, px.data(), px.size());
    return HJR_OK;
}

extern "C" int hjr_load_image_rgba8(const char* path, uint8_t** rgba, int* w, int* h)
{
    if (!path || !rgba || !w || !h) { set_error("hjr_load_image_rgba8: null argument"); return HJR_ERR_ARG; }
    std::vector<uint8_t> px;
    std::string err;
    if (!hjr::read_image_rgba8(path, px, *w, *h, err)) {
        set_error(err);
        return err.rfind("cannot open", 0) == 0 ? HJR_ERR_IO : HJR_ERR_PARSE;
    }
    *rgba = (uint8_t*)malloc(px.size());
    if (!*rgba) { set_error("out of memory"); return HJR_ERR_ARG; }
    memcpy(*rgba, px.data(), px.size());
    return HJR_OK;
}

extern "C" int hjr_load_hdr_rgba32f(const char* path, float** rgba, int* w, int* h)
{
    if (!path || !rgba || !w || !h) { set_error("hjr_load_hdr_rgba32f: null argument"); return HJR_ERR_ARG; }
    std::vector<float> px;
    std::string err;
    if (!hjr::read_hdr_rgba32f(path, px, *w, *h, err)) {
        set_error(err);
        return err.rfind("cannot open", 0) == 0 ? HJR_ERR_IO : HJR_ERR_PARSE;
    }
    *rgba = (float*)malloc(px.size() * sizeof(float));
    if (!*rgba) { set_error("out of memory"); return HJR_ERR_ARG; }
    memcpy(*rgba, px.data(), px.size() * sizeof(float));
    return HJR_OK;
}

extern "C" void hjr_free(void* p) { free(p); }

// ---- pixel-tile shard: 8x8 tiles, tile t -> rank t % world; packed form = the rank's tiles back to back
extern "C" uint32_t hjr_owned_tiles(uint32_t w, uint32_t h, uint32_t rank, uint32_t world)
{
    if (world == 0 || rank >= world) return 0;
    const uint64_t n_tiles = (uint64_t)((w + 7u) / 8u) * ((h + 7u) / 8u);
    return n_tiles > rank ? (uint32_t)((n_tiles - rank + world - 1) / world) : 0u;
}
// boundary granule of sample passes: one work-item chunk, or the whole frame when it is a single chunk
extern "C" uint32_t hjr_sample_granule(uint32_t spp)
{
    if (spp == 0) return 0;
    const uint32_t g = hjr_chunk_spp(spp);
    return g >= spp ? spp : g;
}
template <bool PACK> static int tiles_copy(const float* src, float* dst, uint32_t w, uint32_t h, uint32_t rank, uint32_t world)
{
    if (!src || !dst || w == 0 || h == 0 || world == 0 || rank >= world) { set_error("hjr_pack_tiles / hjr_unpack_tiles: bad argument"); return HJR_ERR_ARG; }
    const uint32_t tiles_x = (w + 7u) / 8u, n = hjr_owned_tiles(w, h, rank, world);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t tx, ty;
        hjr_tile_xy(i * world + rank, tiles_x, &tx, &ty);
        const uint32_t x0 = tx * 8u, y0 = ty * 8u;
        for (uint32_t k = 0; k < 64u; k++) {
            const uint32_t x = x0 + (k & 7u), y = y0 + (k >> 3);
            float* p = PACK ? dst + ((size_t)i * 64 + k) * 4 : nullptr;
            if (x < w && y < h) {
                const size_t f = ((size_t)y * w + x) * 4, q = ((size_t)i * 64 + k) * 4;
                if (PACK) memcpy(dst + q, src + f, 16); else memcpy(dst + f, src + q, 16);
            } else if (PACK) p[0] = p[1] = p[2] = p[3] = 0.0f;
        }
    }
    return HJR_OK;
}
extern "C" int hjr_pack_tiles(const float* frame, uint32_t w, uint32_t h, uint32_t rank, uint32_t world, float* packed) { return tiles_copy<true>(frame, packed, w, h, rank, world); }
extern "C" int hjr_unpack_tiles(const float* packed, uint32_t w, uint32_t h, uint32_t rank, uint32_t world, float* frame) { return tiles_copy<false>(packed, frame, w, h, rank, world); }

// ---- buckets and compositing of render windows (include/henjou_hip.h: hjr_params.window)
static bool bucket_args_ok(uint32_t w, uint32_t h, uint32_t bw, uint32_t bh) { return w && h && bw && bh && bw % HJR_TILE == 0 && bh % HJR_TILE == 0; }
extern "C" uint32_t hjr_bucket_count(uint32_t w, uint32_t h, uint32_t bw, uint32_t bh)
{
    if (!bucket_args_ok(w, h, bw, bh)) return 0;
    const uint64_t n = (uint64_t)((w - 1u) / bw + 1u) * ((h - 1u) / bh + 1u);
    return n > 0xffffffffull ? 0u : (uint32_t)n;
}
extern "C" int hjr_bucket_window(uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint32_t index, uint32_t window[4])
{
    if (!window) { set_error("hjr_bucket_window: null argument"); return HJR_ERR_ARG; }
    if (!bucket_args_ok(w, h, bw, bh)) { set_error("hjr_bucket_window: the frame must not be empty and the bucket sides must be positive multiples of 8"); return HJR_ERR_ARG; }
    const uint32_t nx = (w - 1u) / bw + 1u, n = hjr_bucket_count(w, h, bw, bh);
    if (index >= n) { set_error("hjr_bucket_window: bucket index " + std::to_string(index) + " of " + std::to_string(n)); return HJR_ERR_ARG; }
    const uint32_t bx = index % nx, by = index / nx;
    window[0] = bx * bw; window[1] = by * bh;
    window[2] = w - window[0] > bw ? window[0] + bw : w; // (edge buckets are clipped to the frame)
    window[3] = h - window[1] > bh ? window[1] + bh : h;
    return HJR_OK;
}
namespace hjr {
// the argument rule of hjr_blit_window and hjr_blit_window_device (csrc/hjr_util.hip)
int check_blit_window(const uint32_t window[4], uint32_t w, uint32_t h, const char* who)
{
    if (window[0] < window[2] && window[2] <= w && window[1] < window[3] && window[3] <= h) return HJR_OK;
    set_error(std::string(who) + ": window needs x0 < x1 <= width and y0 < y1 <= height");
    return HJR_ERR_ARG;
}
} // namespace hjr
extern "C" int hjr_blit_window(const float* win, const uint32_t window[4], float* frame, uint32_t w, uint32_t h)
{
    if (!win || !window || !frame) { set_error("hjr_blit_window: null argument"); return HJR_ERR_ARG; }
    if (const int rc = hjr::check_blit_window(window, w, h, "hjr_blit_window")) return rc;
    const uint32_t ww = window[2] - window[0], wh = window[3] - window[1];
    for (uint32_t y = 0; y < wh; y++) memcpy(frame + ((size_t)(window[1] + y) * w + window[0]) * 4, win + (size_t)y * ww * 4, (size_t)ww * 16);
    return HJR_OK;
}

// ---- gathered shards -> frames (include/henjou_hip.h, DESIGN.md §7 "Denoise modes").  The argument rule of hjr_assemble_shards and
// hjr_assemble_shards_device (csrc/hjr_post.hip) in one place: sizes, alignment, and per AOV "source and output both or neither".
namespace hjr {
int check_shards(const hjr_shards& s, uint32_t w, uint32_t h, const void* const out[4], const char* who)
{
    const std::string me = who;
    if (w == 0 || h == 0 || w > 16384 || h > 16384) { set_error(me + ": bad image size"); return HJR_ERR_ARG; }
    if (s.world_size == 0) { set_error(me + ": world_size is 0"); return HJR_ERR_ARG; }
    const void* const src[4] = { s.color, s.albedo, s.normal, s.variance };
    bool any = false;
    for (int k = 0; k < 4; k++) {
        if ((src[k] != nullptr) != (out[k] != nullptr)) { set_error(me + ": an output needs its source block and a source block its output (both NULL or neither)"); return HJR_ERR_ARG; }
        if (k < 3 && src[k] && (((uintptr_t)src[k] | (uintptr_t)out[k]) & 15u)) { set_error(me + ": float4 blocks and frames must be 16-byte aligned"); return HJR_ERR_ARG; }
        if (k == 3 && src[k] && (((uintptr_t)src[k] | (uintptr_t)out[k]) & 3u)) { set_error(me + ": the variance block and frame must be 4-byte aligned"); return HJR_ERR_ARG; }
        any = any || src[k];
    }
    if (!any) { set_error(me + ": no AOV given"); return HJR_ERR_ARG; }
    if (s.rank_stride % 16u) { set_error(me + ": rank_stride must be a multiple of 16"); return HJR_ERR_ARG; }
    // blocks of two ranks must not overlap: rank 0 owns the most tiles
    const uint64_t need = (uint64_t)hjr_owned_tiles(w, h, 0, s.world_size) * 64u * ((s.color || s.albedo || s.normal) ? 16u : 4u);
    if (s.world_size > 1 && s.rank_stride < need) { set_error(me + ": rank_stride is smaller than rank 0's block"); return HJR_ERR_ARG; }
    return HJR_OK;
}
} // namespace hjr
// host form: per pixel the arithmetic of csrc/hjr_shards.hip.h::hjr_assemble_shards_kernel (tile id -> owner and slot; no table of owners)
extern "C" int hjr_assemble_shards(const hjr_shards* shards, uint32_t w, uint32_t h, float* color, float* albedo, float* normal, float* variance)
{
    hjr_shards s;
    const void* const out[4] = { color, albedo, normal, variance };
    if (!hjr::abi_take(shards, s, "hjr_assemble_shards")) return HJR_ERR_ARG;
    if (const int rc = hjr::check_shards(s, w, h, out, "hjr_assemble_shards")) return rc;
    const uint32_t tiles_x = (w + 7u) / 8u;
    const char* const src4[3] = { (const char*)s.color, (const char*)s.albedo, (const char*)s.normal };
    float* const dst4[3] = { color, albedo, normal };
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const uint32_t t = hjr_tile_id(x / 8u, y / 8u, tiles_x);
            const size_t off = (size_t)(t % s.world_size) * s.rank_stride, slot = (size_t)(t / s.world_size) * 64u + (y & 7u) * 8u + (x & 7u), pix = (size_t)y * w + x;
            for (int k = 0; k < 3; k++)
                if (dst4[k]) memcpy(dst4[k] + pix * 4, src4[k] + off + slot * 16, 16);
            if (variance) memcpy(variance + pix, (const char*)s.variance + off + slot * 4, 4);
        }
    return HJR_OK;
}

extern "C" int hjr_float4_to_srgb8(const float* rgba, uint8_t* out, uint32_t n)
{
    if ((!rgba || !out) && n) { set_error("hjr_float4_to_srgb8: null argument"); return HJR_ERR_ARG; }
    hjr::float4_to_srgb8(rgba, out, n);
    return HJR_OK;
}

extern "C" int hjr_tonemap_to_srgb8(const float* rgba, uint8_t* out, uint32_t n, int tonemap)
{
    if ((!rgba || !out) && n) { set_error("hjr_tonemap_to_srgb8: null argument"); return HJR_ERR_ARG; }
    if (tonemap < HJR_TONEMAP_NONE || tonemap > HJR_TONEMAP_ACES) { set_error("hjr_tonemap_to_srgb8: unknown tonemap"); return HJR_ERR_ARG; }
    hjr::tonemap_to_srgb8(rgba, out, n, tonemap);
    return HJR_OK;
}

extern "C" int hjr_write_png(const char* path, const uint8_t* rgba8, uint32_t w, uint32_t h, int flip_y)
{
    if (!path || !rgba8) { set_error("hjr_write_png: null argument"); return HJR_ERR_ARG; }
    std::string err;
    if (!hjr::write_png(path, rgba8, w, h, flip_y != 0, err)) { set_error(err); return HJR_ERR_IO; }
    return HJR_OK;
}

extern "C" int hjr_write_pfm(const char* path, const float* rgba, uint32_t w, uint32_t h)
{
    if (!path || !rgba) { set_error("hjr_write_pfm: null argument"); return HJR_ERR_ARG; }
    std::string err;
    if (!hjr::write_pfm(path, rgba, w, h, err)) { set_error(err); return HJR_ERR_IO; }
    return HJR_OK;
}
