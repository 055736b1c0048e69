// assemble_shards_test <w> <h> <world>: hjr_assemble_shards (host/capi.cpp, compiled in) under AddressSanitizer / UBSan.
// One gathered buffer, per rank colour | albedo | normal | variance, allocated to the byte: it ends with the last slot of the last rank's
// last tile.  Everything hjr_assemble_shards must not read is POISONED, so that touching it is an ASan error: the padding behind a rank's last
// tile (ranks that own fewer tiles than rank 0) and the out-of-image lanes of edge tiles.  (ASan poisons whole aligned 8-byte words: exact for
// the float4 AOVs; of a run of out-of-image variance floats the words that lie wholly inside the run.)  The frames must equal world
// applications of hjr_unpack_tiles per float4 AOV, and for the variance the slot formula written out here; every null / non-null combination
// of the four AOVs is run.
#include <sanitizer/asan_interface.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/henjou_hip.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "assemble_shards_test: %s failed (line %d): %s\n", #c, __LINE__, hjr_last_error()); return 1; } } while (0)

static void tile_xy(uint32_t t, uint32_t tiles_x, uint32_t* tx, uint32_t* ty) // include/henjou_hip.h: t = ty * tiles_x + (tx + ty) % tiles_x
{
    *ty = t / tiles_x;
    const uint32_t c = t % tiles_x, r = *ty % tiles_x;
    *tx = (c + tiles_x - r) % tiles_x;
}

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: assemble_shards_test w h world\n"); return 2; }
    const uint32_t w = (uint32_t)atoi(argv[1]), h = (uint32_t)atoi(argv[2]), world = (uint32_t)atoi(argv[3]);
    const uint32_t tiles_x = (w + 7) / 8;
    const size_t slots0 = (size_t)hjr_owned_tiles(w, h, 0, world) * 64;
    const size_t off[4] = { 0, slots0 * 16, slots0 * 32, slots0 * 48 }, elem[4] = { 16, 16, 16, 4 };
    const size_t stride = slots0 * 52;
    CHECK(stride % 16 == 0);
    const size_t last_slots = (size_t)hjr_owned_tiles(w, h, world - 1, world) * 64;
    const size_t bytes = (size_t)(world - 1) * stride + off[3] + last_slots * 4; // to the byte
    char* buf = (char*)malloc(bytes ? bytes : 1);
    CHECK(buf);
    // fill: slot of pixel (x, y), AOV k -> a value that names it; then poison what has no pixel
    std::vector<char> readable(bytes, 0);
    for (uint32_t r = 0; r < world; r++) {
        const uint32_t n = hjr_owned_tiles(w, h, r, world);
        for (uint32_t i = 0; i < n; i++) {
            uint32_t tx, ty;
            tile_xy(i * world + r, tiles_x, &tx, &ty);
            for (uint32_t l = 0; l < 64; l++) {
                const uint32_t x = tx * 8 + (l & 7), y = ty * 8 + (l >> 3);
                if (x >= w || y >= h) continue;
                for (int k = 0; k < 4; k++) {
                    const size_t at = (size_t)r * stride + off[k] + ((size_t)i * 64 + l) * elem[k];
                    CHECK(at + elem[k] <= bytes);
                    const float v[4] = { (float)x + 0.25f * (float)k, (float)y, (float)r, (float)(k + 1) };
                    memcpy(buf + at, v, elem[k]);
                    memset(readable.data() + at, 1, elem[k]);
                }
            }
        }
    }
    size_t poisoned = 0;
    for (size_t a = 0; a < bytes;) {
        if (readable[a]) { a++; continue; }
        size_t b = a;
        while (b < bytes && !readable[b]) b++;
        const size_t lo = ((uintptr_t)(buf + a) + 7) / 8 * 8 - (uintptr_t)buf, hi = ((uintptr_t)(buf + b)) / 8 * 8 - (uintptr_t)buf;
        if (hi > lo) {
            ASAN_POISON_MEMORY_REGION(buf + lo, hi - lo);
            poisoned += hi - lo;
#if defined(__SANITIZE_ADDRESS__)
            CHECK(__asan_address_is_poisoned(buf + lo) && __asan_address_is_poisoned(buf + hi - 1)); // the trap is armed
#endif
        }
        a = b;
    }
    const size_t npx = (size_t)w * h;
    for (int mask = 1; mask < 16; mask++) {
        hjr_shards s;
        HJR_INIT(s);
        s.world_size = world; s.rank_stride = stride;
        const void** src[4] = { &s.color, &s.albedo, &s.normal, &s.variance };
        std::vector<float> out[4], want[4];
        float* o[4] = { nullptr, nullptr, nullptr, nullptr };
        for (int k = 0; k < 4; k++)
            if (mask & (1 << k)) {
                *src[k] = buf + off[k];
                out[k].assign(npx * elem[k] / 4, -7.0f);
                want[k].assign(npx * elem[k] / 4, -7.0f);
                o[k] = out[k].data();
            }
        CHECK(hjr_assemble_shards(&s, w, h, o[0], o[1], o[2], o[3]) == HJR_OK);
        for (int k = 0; k < 3; k++)
            if (o[k]) {
                // (hjr_unpack_tiles reads in-image slots only, so the poison stays in place for it too)
                for (uint32_t r = 0; r < world; r++)
                    if (hjr_owned_tiles(w, h, r, world)) CHECK(hjr_unpack_tiles((const float*)(buf + (size_t)r * stride + off[k]), w, h, r, world, want[k].data()) == HJR_OK);
                CHECK(memcmp(want[k].data(), out[k].data(), npx * 16) == 0);
                for (size_t i = 0; i < npx; i++) CHECK(out[k][i * 4 + 3] == (float)(k + 1)); // every pixel written
            }
        if (o[3])
            for (uint32_t y = 0; y < h; y++)
                for (uint32_t x = 0; x < w; x++) CHECK(out[3][(size_t)y * w + x] == (float)x + 0.75f);
    }
    ASAN_UNPOISON_MEMORY_REGION(buf, bytes);
    free(buf);
    printf("assemble_shards_test ok: %ux%u world %u, %zu bytes gathered, %zu poisoned\n", w, h, world, bytes, poisoned);
    return 0;
}
