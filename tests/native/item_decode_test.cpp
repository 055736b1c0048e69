// Host enumeration of the megakernel's work-item queue (csrc/hjr_layout.h: hjr_item_chunks, hjr_item_count, hjr_decode_range,
// hjr_item_word, hjr_item_last_chunk) exactly as the kernel walks it: a wave decodes 64 aligned items, a lane takes one, renders the
// chunk in its item word, and at the end of a chunk either gives the pixel up (last chunk of the item) or goes on with chunk + 1.
// For tile grids 1x1, 3x2, 5x3; world 1, 2, 3 (every rank); pass_chunks 1, 2, 3, 4, 6, 8 at chunk0 0 and 1; requested item_chunks 1, 2, 4, 8;
// plain and permuted tile lists:
//   * the effective r is a power of two, <= the request, divides pass_chunks, and no larger power of two does;
//   * the item count is owned tiles * (pass_chunks / r) * 64, what hjr_render.hip sizes the queue for;
//   * every (owned tile, chunk of the pass, pixel) is rendered exactly once, and nothing else is;
//   * the chunks of an item are r consecutive chunks of one pixel, aligned to r from chunk0.
// Build: g++ -O1 -std=c++17 tests/native/item_decode_test.cpp -o item_decode_test
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <vector>

#include "../../henjou-renderer_amd/csrc/hjr_layout.h"

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "item_decode_test: %s failed (line %d): ", #cond, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

static int run_case(uint32_t tiles_x, uint32_t tiles_y, uint32_t world, uint32_t rank, uint32_t pass_chunks, uint32_t chunk0, uint32_t request, bool permuted)
{
    const uint32_t r = hjr_item_chunks(request, pass_chunks);
    CHECK(r >= 1 && (r & (r - 1)) == 0 && r <= request && pass_chunks % r == 0, "request %u pass_chunks %u -> r %u", request, pass_chunks, r);
    CHECK(r * 2 > request || pass_chunks % (r * 2) != 0, "request %u pass_chunks %u -> r %u is not the largest", request, pass_chunks, r);
    // this rank's tiles in the order of their ids (tile t is rank t % world's (t / world)-th tile)
    const uint32_t n_tiles = tiles_x * tiles_y;
    std::vector<uint32_t> owned_ids;
    for (uint32_t t = rank; t < n_tiles; t += world) owned_ids.push_back(t);
    const uint64_t owned = owned_ids.size();
    std::vector<uint32_t> order(owned_ids.rbegin(), owned_ids.rend()); // a tile list other than the plain one: reversed
    const uint64_t n_items = hjr_item_count(owned, pass_chunks, r);
    CHECK(n_items == owned * pass_chunks * 64u / r && n_items % 64u == 0, "n_items %llu", (unsigned long long)n_items);
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, int> seen; // (px, py, chunk) -> times rendered
    for (uint32_t base = 0; base < n_items; base += 64u) {
        const uint32_t word = hjr_decode_range(base, pass_chunks, chunk0, r, tiles_x, world, rank, permuted ? order.data() : nullptr);
        for (uint32_t q = base; q < base + 64u; q++) {
            uint32_t item = hjr_item_word(word, q);
            const uint32_t px = item & 0x1fffu, py = (item >> 13) & 0x1fffu, first = item >> 26;
            CHECK(px / HJR_TILE < tiles_x && py / HJR_TILE < tiles_y, "item %u: pixel (%u, %u) outside the grid", q, px, py);
            CHECK(hjr_tile_id(px / HJR_TILE, py / HJR_TILE, tiles_x) % world == rank, "item %u: tile of another rank", q);
            CHECK((px & 7u) == (q & 7u) && (py & 7u) == ((q >> 3) & 7u), "item %u: pixel in tile", q);
            CHECK((first - chunk0) % r == 0, "item %u: first chunk %u is not the start of a group", q, first);
            uint32_t walked = 0;
            for (;;) { // the lane's walk: write the chunk out, then stop or move the item word on (hjr_kernel.hip.h: close_sample / write_out)
                const uint32_t chunk = item >> 26;
                CHECK(chunk >= chunk0 && chunk < chunk0 + pass_chunks, "item %u: chunk %u outside [%u, %u)", q, chunk, chunk0, chunk0 + pass_chunks);
                CHECK(chunk == first + walked && (item & 0x3ffffffu) == (hjr_item_word(word, q) & 0x3ffffffu), "item %u: chunks not consecutive / pixel moved", q);
                seen[std::make_tuple(px, py, chunk)]++;
                walked++;
                if (hjr_item_last_chunk(chunk, chunk0, r)) break;
                CHECK(walked < 64u, "item %u never ends", q);
                item += 1u << 26;
            }
            CHECK(walked == r, "item %u: %u chunks, expected %u", q, walked, r);
        }
    }
    CHECK(seen.size() == owned * 64u * pass_chunks, "covered %zu of %llu", seen.size(), (unsigned long long)(owned * 64u * pass_chunks));
    for (const auto& kv : seen) CHECK(kv.second == 1, "(%u, %u) chunk %u rendered %d times", std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first), kv.second);
    for (uint32_t t : owned_ids) { // nothing missing: every pixel and chunk of every owned tile
        uint32_t tx, ty;
        hjr_tile_xy(t, tiles_x, &tx, &ty);
        for (uint32_t j = 0; j < 64u; j++)
            for (uint32_t k = chunk0; k < chunk0 + pass_chunks; k++)
                CHECK(seen.count(std::make_tuple(tx * 8u + (j & 7u), ty * 8u + (j >> 3), k)) == 1, "tile %u pixel %u chunk %u not rendered", t, j, k);
    }
    return 0;
}

int main()
{
    const uint32_t grids[3][2] = { { 1, 1 }, { 3, 2 }, { 5, 3 } }, chunks[6] = { 1, 2, 3, 4, 6, 8 }, requests[4] = { 1, 2, 4, 8 };
    int cases = 0;
    for (const auto& g : grids)
        for (uint32_t world = 1; world <= 3; world++)
            for (uint32_t rank = 0; rank < world; rank++)
                for (uint32_t pc : chunks)
                    for (uint32_t chunk0 = 0; chunk0 <= 1; chunk0++)
                        for (uint32_t req : requests)
                            for (int permuted = 0; permuted <= 1; permuted++, cases++)
                                if (run_case(g[0], g[1], world, rank, pc, chunk0, req, permuted != 0)) {
                                    fprintf(stderr, "  case: grid %ux%u world %u rank %u pass_chunks %u chunk0 %u request %u permuted %d\n", g[0], g[1], world, rank, pc, chunk0, req, permuted);
                                    return 1;
                                }
    // the effective group lengths the issue names
    if (hjr_item_chunks(8, 32) != 8 || hjr_item_chunks(4, 3) != 1 || hjr_item_chunks(4, 6) != 2 || hjr_item_chunks(2, 4) != 2 || hjr_item_chunks(8, 4) != 4 || hjr_item_chunks(1, 8) != 1) {
        fprintf(stderr, "item_decode_test: hjr_item_chunks\n");
        return 1;
    }
    printf("item_decode_test ok: %d cases\n", cases);
    return 0;
}
