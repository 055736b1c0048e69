// Stand-alone check (CPU only) of henjou-renderer_amd/host/render_job.hpp: the layout of the key table, the option lists for_each_option
// gives the three scopes, the refusals of job_check, the pass split and the PNG names.  The fields are filled here with the literal bits of
// the documented layout (include/henjou_hip.h), not through the table, so a row that moves shows.  Prints "ends <spp> <passes> <ends...>" for
// a small grid (tests/test_render_job_host.py compares them with the Python split) and "render_job_test ok".
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../henjou-renderer_amd/host/options.hpp"
#include "../../henjou-renderer_amd/host/render_job.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

typedef std::vector<std::pair<std::string, int>> List;
static List list_of(const hjr_render_option& o, hjr::JobScope s)
{
    List l;
    CHECK(hjr::for_each_option(o, s, [&](const char* k, int v) { l.push_back({ k, v }); return 0; }) == 0);
    return l;
}
static hjr_render_option everything_on(int mode)
{
    hjr_render_option o;
    HJR_INIT(o);
    o.render_mode = mode;
    o.image_width = 75; o.image_height = 41; o.passes = 1;
    o.force_rebuild = 3;
    o.device_bvh = 1 + 5;
    o.device_bvh_opt = 2 | 0x100 | 0x200 | 0x400 | 0x800 | (3 << 12) | (4 << 16);
    o.denoise_variance = 2;
    return o;
}
static std::string refusal(const hjr_render_option& o)
{
    hjr::Job job;
    std::string text;
    return hjr::job_check(o, job, text) ? "" : text;
}

int main()
{
    using namespace hjr;
    const std::vector<KeyRow>& t = key_table();

    // ---- table layout
    CHECK(t.size() == 13);
    for (size_t i = 0; i < t.size(); i++) {
        const KeyRow& r = t[i];
        const int oi = opt_find(r.key);
        CHECK(oi >= 0); // every key sets the context option of its name
        if (oi < 0) continue;
        const long long largest = r.read == READ_FLAG || r.read == READ_BOOL ? 1 : opt_table()[oi].hi;
        if (r.enc == ENC_BITS) {
            CHECK(r.width >= 1 && r.shift + r.width <= 31);
            CHECK(largest < (1ll << r.width));
        } else CHECK(1 + largest < (1ll << 31));
        size_t n_parse = 0;
        for (const KeyRow& q : t) {
            if (q.parse == i) n_parse++; // the parse turns are a permutation of the rows
            if (&q == &r || q.field != r.field) continue;
            if (r.enc == ENC_BITS) {
                CHECK(q.enc == ENC_BITS); // a field whose value is encoded as a whole holds no bit rows
                const long long mr = ((1ll << r.width) - 1) << r.shift, mq = ((1ll << q.width) - 1) << q.shift;
                CHECK((mr & mq) == 0);
            }
        }
        CHECK(n_parse == 1);
        if (r.needs) {
            CHECK(strcmp(key_row(r.needs).key, r.needs) == 0);
            CHECK(key_row(r.needs).parse < r.parse); // the key it needs has been read when it is checked
        }
    }
    // put then get, one key at a time at its largest value
    for (const KeyRow& r : t) {
        hjr_render_option o;
        HJR_INIT(o);
        const int largest = r.read == READ_FLAG || r.read == READ_BOOL ? 1 : opt_table()[opt_find(r.key)].hi;
        key_put(o, r, largest);
        CHECK(key_get(o, r) == largest);
    }

    // ---- for_each_option: what hjr_render_file and the rank path of henjou_cli set, in their order
    const List single = { { "force_rebuild", 1 }, { "verbose", 1 }, { "device_bvh", 1 }, { "device_bvh_refit", 5 }, { "device_bvh_opt", 2 },
                          { "device_bvh_instances", 1 }, { "device_bvh_graft", 1 }, { "denoise_variance", 1 }, { "denoise_temporal", 1 },
                          { "denoise_variance_spatial", 1 }, { "upscale_guided", 1 }, { "denoise_temporal_coverage", 3 }, { "firefly_clamp", 4 } };
    const List rank0(single.begin() + 1, single.end()); // no "force_rebuild" on the rank path
    const List rank1 = { { "verbose", 1 }, { "device_bvh", 1 }, { "device_bvh_refit", 5 }, { "device_bvh_opt", 2 }, { "device_bvh_instances", 1 },
                         { "device_bvh_graft", 1 }, { "firefly_clamp", 4 } }; // no filter key either
    for (int mode : { HJR_MODE_DENOISE, HJR_MODE_DENOISE_UPSCALE2X }) {
        const hjr_render_option o = everything_on(mode);
        CHECK(list_of(o, single_process()) == single);
        CHECK(list_of(o, rank_of_world(0)) == rank0);
        CHECK(list_of(o, rank_of_world(1)) == rank1);
    }
    {
        const hjr_render_option o = everything_on(HJR_MODE_DEFAULT); // no filter: "denoise_variance" and "denoise_temporal" drop out
        List s = single, r0 = rank0;
        s.erase(s.begin() + 7, s.begin() + 9);
        r0.erase(r0.begin() + 6, r0.begin() + 8);
        CHECK(list_of(o, single_process()) == s);
        CHECK(list_of(o, rank_of_world(0)) == r0);
        CHECK(list_of(o, rank_of_world(1)) == rank1);
        hjr_render_option v = everything_on(HJR_MODE_DENOISE);
        v.denoise_variance = 1; v.device_bvh = 1; v.force_rebuild = 2; v.device_bvh_opt = 0;
        CHECK((list_of(v, single_process()) == List{ { "verbose", 1 }, { "device_bvh", 1 }, { "denoise_variance", 1 } }));
        hjr_render_option z;
        HJR_INIT(z);
        CHECK(list_of(z, single_process()).empty() && list_of(z, rank_of_world(0)).empty() && list_of(z, rank_of_world(3)).empty());
        int calls = 0;
        CHECK(for_each_option(everything_on(HJR_MODE_DENOISE), single_process(), [&](const char*, int) { return ++calls == 3 ? -7 : 0; }) == -7 && calls == 3);
    }

    // ---- job_check: the four refusals in their order, and the sizes
    const char* const MODE = "Render_mode must be Default, Denoise or DenoiseUpScale2X (Debug is declared but unused by the reference)";
    const char* const TEMPORAL = "\"denoise_temporal\" cannot be combined with \"noise_threshold\": an adaptive frame that stops early never reaches the sample pass that advances the history";
    const char* const FIREFLY = "\"firefly_clamp\" cannot be combined with \"passes\" > 1 or \"noise_threshold\": the clamp needs every chunk sum of a pixel, and a frame rendered in sample passes keeps running sums only";
    const char* const SMALL = "image too small for DenoiseUpScale2X";
    {
        hjr_render_option o = everything_on(HJR_MODE_DENOISE);
        CHECK(refusal(o) == "");
        o.render_mode = HJR_MODE_DEBUG;
        CHECK(refusal(o) == MODE);
        o.noise_threshold = 0.05f; o.image_width = 1; // every later refusal too: the first one is reported
        CHECK(refusal(o) == MODE);
        o.render_mode = HJR_MODE_DENOISE_UPSCALE2X;
        CHECK(refusal(o) == TEMPORAL);
        o.denoise_variance = 1;
        CHECK(refusal(o) == FIREFLY);
        o.noise_threshold = 0.0f; o.passes = 2;
        CHECK(refusal(o) == FIREFLY);
        o.passes = 1;
        CHECK(refusal(o) == SMALL);
        o.device_bvh_opt = 0; o.passes = 64; o.noise_threshold = 0.5f; o.image_width = 75; // without the clamp, passes and a threshold are fine
        CHECK(refusal(o) == "");
        o.render_mode = HJR_MODE_DEFAULT; o.denoise_variance = 2; // Default mode ignores "denoise_temporal"
        CHECK(refusal(o) == "");
        for (int mode : { HJR_MODE_DEFAULT, HJR_MODE_DENOISE, HJR_MODE_DENOISE_UPSCALE2X })
            for (uint32_t side : { 75u, 1u }) {
                hjr_render_option q = everything_on(mode);
                q.image_width = side; q.image_height = side == 75u ? 41u : 1u;
                Job job;
                std::string text;
                const bool ok = job_check(q, job, text);
                const bool half = mode == HJR_MODE_DENOISE_UPSCALE2X;
                CHECK(ok == !(half && side == 1u) && (ok || text == SMALL));
                CHECK(job.out_w == side && job.out_h == q.image_height);
                CHECK(job.w == (half ? side / 2u : side) && job.h == (half ? q.image_height / 2u : q.image_height));
                CHECK(job.denoise == (mode != HJR_MODE_DEFAULT) && job.with_var == job.denoise && job.temporal == job.denoise && job.firefly == 4 && !job.adaptive);
            }
        hjr_render_option q = everything_on(HJR_MODE_DENOISE_UPSCALE2X);
        Job job;
        std::string text;
        CHECK(job_check(q, job, text) && job.w == 37 && job.h == 20 && job.out_w == 75 && job.out_h == 41);
    }

    // ---- pass_ends
    for (uint32_t spp = 1; spp <= 300; spp++)
        for (uint32_t n = 1; n <= 64; n++) {
            const std::vector<uint32_t> e = pass_ends(spp, n);
            const uint32_t g = hjr_sample_granule(spp);
            bool ok = !e.empty() && e.size() <= n && e.back() == spp && g > 0;
            for (size_t k = 0; ok && k < e.size(); k++) ok = e[k] > (k ? e[k - 1] : 0u) && (k + 1 == e.size() || e[k] % g == 0);
            if (!ok) { printf("FAILED pass_ends(%u, %u)\n", spp, n); fails++; }
        }
    for (uint32_t spp : { 1u, 7u, 12u, 64u, 100u, 255u, 256u, 300u, 1000u, 4096u })
        for (uint32_t n : { 1u, 2u, 3u, 8u, 64u }) {
            printf("ends %u %u", spp, n);
            for (uint32_t e : pass_ends(spp, n)) printf(" %u", e);
            printf("\n");
        }

    // ---- <image_name>_<fff>.png
    {
        hjr_render_option o;
        HJR_INIT(o);
        strcpy(o.image_name, "out/cornel");
        CHECK(frame_png_name(o, 0) == "out/cornel_000.png" && frame_png_name(o, 7) == "out/cornel_007.png" && frame_png_name(o, 12) == "out/cornel_012.png");
        CHECK(frame_png_name(o, 123) == "out/cornel_123.png" && frame_png_name(o, 1234) == "out/cornel_1234.png");
    }
    if (fails == 0) printf("render_job_test ok: %zu keys\n", t.size());
    return fails ? 1 : 0;
}
