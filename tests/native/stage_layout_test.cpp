// Host test of the staging arena (henjou-renderer_amd/host/stage_layout.hpp): the cursor and the item list (StageLayout) that HostStage
// (csrc/hjr_device_internal.h) lays the temporary device buffer of a host-buffer entry point out with.  Built with
// -fsanitize=address,undefined by tests/test_stage_layout_native.py; a stand-alone program.
//   * every offset is a multiple of its item's alignment;
//   * no two items of positive size overlap, and a zero-byte item takes nothing;
//   * the total covers the last item;
//   * resolve() writes base + offset into every slot, whatever the slot's pointer type.
// Cases: mixed alignments with a 4-byte image of an odd number of floats in front of an 8-byte and a 16-byte one, zero-byte items, a single
// item, and the item list of hjr_temporal_accumulate_response (csrc/hjr_post.hip) at 7 x 5 pixels with 3 instances, with and without a
// previous side, with moments and response on.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../henjou-renderer_amd/host/stage_layout.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

struct Want { size_t bytes, align; };

// lays `want` out, checks the three properties and the resolved pointers; returns the total
static size_t check_layout(const char* name, const std::vector<Want>& want)
{
    hjr::StageLayout lay;
    std::vector<const float*> slots(want.size(), nullptr); // (any object-pointer type: the entry points mix const float*, float4*, void*)
    for (size_t i = 0; i < want.size(); i++) lay.add(slots[i], nullptr, nullptr, want[i].bytes, want[i].align);
    CHECK(lay.items.size() == want.size(), "%s: %zu items", name, lay.items.size());
    size_t end = 0;
    for (size_t i = 0; i < want.size(); i++) {
        const hjr::StageLayout::Item& a = lay.items[i];
        CHECK(a.bytes == want[i].bytes, "%s: item %zu keeps its size", name, i);
        CHECK(a.off % want[i].align == 0, "%s: item %zu at %zu is not a multiple of %zu", name, i, a.off, want[i].align);
        if (a.bytes) CHECK(a.off + a.bytes <= lay.total(), "%s: item %zu [%zu, %zu) ends behind the total %zu", name, i, a.off, a.off + a.bytes, lay.total());
        if (a.off + a.bytes > end && a.bytes) end = a.off + a.bytes;
        for (size_t j = 0; j < i; j++) {
            const hjr::StageLayout::Item& b = lay.items[j];
            if (a.bytes && b.bytes) CHECK(a.off >= b.off + b.bytes || b.off >= a.off + a.bytes, "%s: items %zu and %zu overlap", name, j, i);
        }
    }
    CHECK(lay.total() == end, "%s: the total %zu is the end of the last item %zu", name, lay.total(), end);
    // the buffer the layout asks for (and the alignment gap a trailing zero-byte item may point into), written through every resolved
    // pointer: the sanitizer sees an item that leaves it
    std::vector<unsigned char> buf(lay.total() + 16);
    lay.resolve(buf.data());
    for (size_t i = 0; i < want.size(); i++) {
        unsigned char* const p = (unsigned char*)slots[i];
        CHECK(p == buf.data() + lay.items[i].off, "%s: slot %zu is base + offset", name, i);
        for (size_t k = 0; k < want[i].bytes; k++) p[k] = (unsigned char)i;
    }
    for (size_t i = 0; i < want.size(); i++)
        for (size_t k = 0; k < want[i].bytes; k++) CHECK(((unsigned char*)slots[i])[k] == (unsigned char)i, "%s: item %zu was written over", name, i);
    return lay.total();
}

// the item list of hjr_temporal_accumulate_response: per side M, M^-1, the G-buffer, colour, variance (prev: history, moments), then the outputs
static std::vector<Want> temporal_items(size_t npx, size_t n_inst, bool have_prev, bool moments, bool response, size_t gbuf_px)
{
    const size_t nx = n_inst * 48, mom = moments ? npx * 8 : 0, resp = response ? npx * 4 : 0;
    std::vector<Want> w;
    for (int i = have_prev ? 0 : 1; i < 2; i++) {
        w.push_back({ nx, 4 }); w.push_back({ nx, 4 });
        w.push_back({ npx * gbuf_px, 16 });
        w.push_back({ npx * 16, 16 }); w.push_back({ npx * 4, 4 });
        if (i == 0) w.push_back({ npx * 4, 4 });
        if (i == 0 && mom) w.push_back({ mom, 8 });
    }
    w.push_back({ npx * 16, 16 }); w.push_back({ npx * 4, 4 }); w.push_back({ npx * 4, 4 });
    if (mom) w.push_back({ mom, 8 });
    if (resp) w.push_back({ resp, 4 });
    return w;
}

int main()
{
    { // the cursor alone
        hjr::StageLayout c;
        CHECK(c.total() == 0, "an empty cursor");
        CHECK(c.take(0, 16) == 0 && c.total() == 0, "a zero-byte request at the start moves nothing");
        CHECK(c.take(20, 4) == 0 && c.total() == 20, "five floats");
        CHECK(c.take(0, 16) == 32 && c.total() == 20, "a zero-byte request returns the aligned offset and moves nothing");
        CHECK(c.take(8, 8) == 24 && c.total() == 32, "a float2 behind five floats");
        CHECK(c.take(16, 16) == 32 && c.total() == 48, "a float4 behind it");
        CHECK(c.take(4, 4) == 48 && c.take(16, 16) == 64 && c.total() == 80, "a float, then a float4");
    }
    // 35 floats (7 x 5 pixels, one float each: 140 bytes, a multiple of neither 8 nor 16), then float2 and float4 images
    CHECK(check_layout("mixed", { { 35 * 4, 4 }, { 35 * 8, 8 }, { 35 * 16, 16 }, { 4, 4 }, { 35 * 16, 16 }, { 35 * 4, 4 }, { 35 * 8, 8 } }) > 0, "mixed");
    CHECK(check_layout("zero-byte items", { { 0, 4 }, { 140, 4 }, { 0, 16 }, { 0, 8 }, { 280, 8 }, { 0, 16 } }) == 144 + 280, "zero-byte items take nothing");
    CHECK(check_layout("only zero-byte items", { { 0, 4 }, { 0, 16 } }) == 0, "nothing staged");
    CHECK(check_layout("a single item", { { 140, 4 } }) == 140, "a single item is its size");
    CHECK(check_layout("a single aligned item", { { 560, 16 } }) == 560, "a single item is its size");
    for (const size_t gbuf_px : { (size_t)32, (size_t)48 }) // (the record's size is a multiple of 16; both are tried)
        for (const bool have_prev : { false, true })
            for (const bool on : { false, true }) {
                const std::vector<Want> w = temporal_items(7 * 5, 3, have_prev, on, on, gbuf_px);
                size_t sum = 0;
                for (const Want& x : w) sum += x.bytes;
                const size_t total = check_layout("hjr_temporal_accumulate_response", w);
                CHECK(total >= sum && total < sum + 16 * w.size(), "temporal: the total %zu holds the images' %zu bytes and padding only", total, sum);
            }
    check_layout("hjr_temporal_accumulate_response, no instances", temporal_items(7 * 5, 0, true, true, true, 32));
    if (failures) { printf("stage_layout_test: %d failures\n", failures); return 1; }
    printf("stage_layout_test ok\n");
    return 0;
}
