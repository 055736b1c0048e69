// Stand-alone check (CPU only, built with -fsanitize=address,undefined by tests/test_window_host.py) of the host code of the render window:
// hjr_bucket_count / hjr_bucket_window, hjr_blit_window, and the "window" / "bucket" keys of the "Henjou_HIP" section as callers with
// hjr_render_option, hjr_render_option_window and other struct sizes receive them through the two loader entry points.  Every buffer is allocated with exactly the bytes
// its caller owns.  argv[1]: a render_option.json with "window": [8, 16, 24, 27] and "bucket": [16, 8].  Prints "window_test ok".
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/henjou_hip.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static void check_buckets(uint32_t w, uint32_t h, uint32_t bw, uint32_t bh)
{
    const uint32_t n = hjr_bucket_count(w, h, bw, bh);
    CHECK(n == ((w + bw - 1) / bw) * ((h + bh - 1) / bh));
    std::vector<int> cover((size_t)w * h, 0);
    uint32_t last[4] = { 0, 0, 0, 0 };
    for (uint32_t i = 0; i < n; i++) {
        uint32_t* win = (uint32_t*)malloc(16); // exactly four words
        CHECK(hjr_bucket_window(w, h, bw, bh, i, win) == HJR_OK);
        CHECK(win[0] % 8 == 0 && win[1] % 8 == 0 && win[0] < win[2] && win[1] < win[3] && win[2] <= w && win[3] <= h);
        CHECK(win[2] - win[0] <= bw && win[3] - win[1] <= bh);
        if (i) CHECK(win[1] > last[1] || (win[1] == last[1] && win[0] > last[0])); // row-major
        for (uint32_t y = win[1]; y < win[3]; y++)
            for (uint32_t x = win[0]; x < win[2]; x++) cover[(size_t)y * w + x]++;
        memcpy(last, win, 16);
        free(win);
    }
    for (int c : cover) CHECK(c == 1);
    uint32_t win[4] = { 7, 7, 7, 7 };
    CHECK(hjr_bucket_window(w, h, bw, bh, n, win) == HJR_ERR_ARG && win[0] == 7 && win[3] == 7);
}

int main(int argc, char** argv)
{
    check_buckets(43, 29, 16, 8);
    check_buckets(43, 29, 8, 8);
    check_buckets(43, 29, 48, 32);
    check_buckets(8, 8, 8, 8);
    uint32_t win[4];
    CHECK(hjr_bucket_count(43, 29, 12, 8) == 0 && hjr_bucket_count(43, 29, 16, 0) == 0 && hjr_bucket_count(0, 29, 16, 8) == 0);
    CHECK(hjr_bucket_window(43, 29, 12, 8, 0, win) == HJR_ERR_ARG);
    CHECK(hjr_bucket_window(43, 29, 16, 4, 0, win) == HJR_ERR_ARG);
    CHECK(hjr_bucket_window(43, 29, 16, 8, 0, nullptr) == HJR_ERR_ARG);

    { // blit: buffers of exactly the window's and the frame's size
        const uint32_t W = 43, H = 29, w[4] = { 16, 8, 43, 29 };
        const uint32_t ww = w[2] - w[0], wh = w[3] - w[1];
        float* img = (float*)malloc((size_t)ww * wh * 16);
        float* frame = (float*)malloc((size_t)W * H * 16);
        for (size_t i = 0; i < (size_t)ww * wh * 4; i++) img[i] = (float)i;
        for (size_t i = 0; i < (size_t)W * H * 4; i++) frame[i] = -1.0f;
        CHECK(hjr_blit_window(img, w, frame, W, H) == HJR_OK);
        for (uint32_t y = 0; y < H; y++)
            for (uint32_t x = 0; x < W; x++)
                for (int k = 0; k < 4; k++) {
                    const bool in = x >= w[0] && x < w[2] && y >= w[1] && y < w[3];
                    CHECK(frame[((size_t)y * W + x) * 4 + k] == (in ? (float)((((size_t)(y - w[1])) * ww + (x - w[0])) * 4 + k) : -1.0f));
                }
        const uint32_t bad[3][4] = { { 16, 8, 44, 29 }, { 16, 8, 16, 29 }, { 16, 30, 43, 29 } };
        for (const auto& b : bad) CHECK(hjr_blit_window(img, b, frame, W, H) == HJR_ERR_ARG);
        CHECK(hjr_blit_window(nullptr, w, frame, W, H) == HJR_ERR_ARG);
        free(img);
        free(frame);
    }

    if (argc > 1) { // the two keys through callers of every size
        hjr_render_option_window* lo = (hjr_render_option_window*)malloc(sizeof(hjr_render_option_window));
        HJR_INIT_WINDOW(*lo, o);
        CHECK(hjr_load_render_option_window(argv[1], &lo->o) == HJR_OK);
        CHECK(lo->o.struct_size == sizeof(hjr_render_option_window) && sizeof(hjr_render_option_window) == sizeof(hjr_render_option) + 24);
        CHECK(offsetof(hjr_render_option_window, window) == sizeof(hjr_render_option) && offsetof(hjr_params_window, window) == sizeof(hjr_params));
        CHECK(lo->window[0] == 8 && lo->window[1] == 16 && lo->window[2] == 24 && lo->window[3] == 27 && lo->bucket[0] == 16 && lo->bucket[1] == 8);
        // the short struct, through both entry points: nothing behind it is written (ASan), the fields are the long struct's
        for (int which = 0; which < 2; which++) {
            hjr_render_option* sh = (hjr_render_option*)malloc(sizeof(hjr_render_option));
            HJR_INIT(*sh);
            CHECK((which ? hjr_load_render_option_window(argv[1], sh) : hjr_load_render_option(argv[1], sh)) == HJR_OK);
            CHECK(sh->struct_size == sizeof(hjr_render_option));
            CHECK(memcmp((unsigned char*)sh + 4, (unsigned char*)lo + 4, sizeof(hjr_render_option) - 4) == 0);
            free(sh);
        }
        // a struct that ends inside the window: it receives the words it has
        const size_t part_size = sizeof(hjr_render_option) + 8;
        unsigned char* part = (unsigned char*)malloc(part_size);
        memset(part, 0, part_size);
        const uint32_t pn = (uint32_t)part_size;
        memcpy(part, &pn, 4);
        CHECK(hjr_load_render_option_window(argv[1], (hjr_render_option*)part) == HJR_OK);
        CHECK(memcmp(part + 4, (unsigned char*)lo + 4, part_size - 4) == 0);
        // a longer caller: the tail stays as it was; hjr_load_render_option never writes behind sizeof(hjr_render_option)
        for (int which = 0; which < 2; which++) {
            const size_t known = which ? sizeof(hjr_render_option_window) : sizeof(hjr_render_option);
            const size_t long_size = sizeof(hjr_render_option_window) + 64;
            unsigned char* lg = (unsigned char*)malloc(long_size);
            memset(lg, 0xEE, long_size);
            const uint32_t m = (uint32_t)long_size;
            memcpy(lg, &m, 4);
            CHECK((which ? hjr_load_render_option_window(argv[1], (hjr_render_option*)lg) : hjr_load_render_option(argv[1], (hjr_render_option*)lg)) == HJR_OK);
            CHECK(memcmp(lg + 4, (unsigned char*)lo + 4, known - 4) == 0);
            for (size_t i = known; i < long_size; i++) CHECK(lg[i] == 0xEE);
            free(lg);
        }
        free(lo); free(part);
    }
    if (fails) { printf("window_test: %d checks failed\n", fails); return 1; }
    printf("window_test ok\n");
    return 0;
}
