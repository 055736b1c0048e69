// CPU restatement of the guided 2x upscale (hjr_upscale_guided), written from the specification in the header comment of
// henjou-renderer_amd/csrc/hjr_denoise.hip.h, not from the kernel: the GPU kernel must equal it bit for bit
// (tests/test_gpu_upscale_guided.py), and the quality rehearsal of DESIGN.md §11.4 runs it on oracle frames.  Built by the tests with
// g++ -O2 -ffp-contract=off: fp32, every operation as written.
//
//   upscale_guided_ref IW IH OW OH in.bin out.bin [k_plane k_normal]
//     in.bin   camera (13 float32: pos, dir, up, right, f), colour [IH][IW][4] float32, low-resolution records [IH][IW], output-size
//              records [OH][OW]; a record is 48 bytes: uint32 prim, inst; float32 t, b1, b2, pos[3], ng[3]; uint32 pad
//     out.bin  float32 image [OH][OW][4], then int32 [OH][OW]: how many of the pixel's four taps are valid
//     k_plane, k_normal   override the constants (the rehearsal's one re-tune); default 1 and 0.9
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Rec { uint32_t prim, inst; float t, b1, b2; float pos[3]; float ng[3]; uint32_t pad; };
struct Px { float c[4]; };
static_assert(sizeof(Rec) == 48 && sizeof(Px) == 16, "layout");

static const uint32_t MISS = 0xffffffffu;
static float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

int main(int argc, char** argv)
{
    if (argc < 7) { fprintf(stderr, "usage: upscale_guided_ref IW IH OW OH in.bin out.bin [k_plane k_normal]\n"); return 2; }
    const int iw = atoi(argv[1]), ih = atoi(argv[2]), ow = atoi(argv[3]), oh = atoi(argv[4]);
    const float k_plane = argc > 8 ? (float)atof(argv[7]) : 1.0f, k_normal = argc > 8 ? (float)atof(argv[8]) : 0.9f;
    if (iw <= 0 || ih <= 0 || ow / 2 != iw || oh / 2 != ih) { fprintf(stderr, "upscale_guided_ref: bad sizes\n"); return 2; }
    const size_t n_in = (size_t)iw * ih, n_out = (size_t)ow * oh;
    float cam[13];
    std::vector<Px> color(n_in), out(n_out);
    std::vector<Rec> lo(n_in), hi(n_out);
    std::vector<int32_t> count(n_out);
    FILE* f = fopen(argv[5], "rb");
    if (!f || fread(cam, 4, 13, f) != 13 || fread(color.data(), 16, n_in, f) != n_in || fread(lo.data(), 48, n_in, f) != n_in || fread(hi.data(), 48, n_out, f) != n_out) {
        fprintf(stderr, "upscale_guided_ref: cannot read %s\n", argv[5]);
        return 1;
    }
    fclose(f);
    const float* cam_pos = cam;
    const float cam_f = cam[12];
    for (int Y = 0; Y < oh; Y++)
        for (int X = 0; X < ow; X++) {
            // 1. taps: the source coordinate (X + 0.5) / 2 - 0.5 lies a quarter or three quarters of the way from texel x0 to x0 + 1
            const bool odd_x = (X % 2) != 0, odd_y = (Y % 2) != 0;
            const int x0 = odd_x ? X / 2 : X / 2 - 1, y0 = odd_y ? Y / 2 : Y / 2 - 1;
            const float fx = odd_x ? 0.25f : 0.75f, fy = odd_y ? 0.25f : 0.75f, gx = 1.0f - fx, gy = 1.0f - fy;
            const int xs[2] = { clampi(x0, 0, iw - 1), clampi(x0 + 1, 0, iw - 1) }, ys[2] = { clampi(y0, 0, ih - 1), clampi(y0 + 1, 0, ih - 1) };
            size_t tap[4];
            float w[4];
            for (int k = 0; k < 4; k++) {
                tap[k] = (size_t)ys[k / 2] * iw + xs[k % 2];
                w[k] = ((k % 2) ? fx : gx) * ((k / 2) ? fy : gy);
            }
            // 2. / 3. records and validity
            const Rec& G = hi[(size_t)Y * ow + X];
            float view[3];
            for (int i = 0; i < 3; i++) view[i] = G.pos[i] - cam_pos[i];
            const float vv = dot3(view, view), fh = cam_f * (float)ih, fp2 = (vv * 4.0f) / (fh * fh), nn = dot3(G.ng, G.ng);
            bool valid[4];
            int n_valid = 0;
            for (int k = 0; k < 4; k++) {
                const Rec& T = lo[tap[k]];
                if (G.prim == MISS) valid[k] = T.prim == MISS;
                else if (T.prim == MISS || T.inst != G.inst) valid[k] = false;
                else {
                    float D[3];
                    for (int i = 0; i < 3; i++) D[i] = T.pos[i] - G.pos[i];
                    const float nd = dot3(G.ng, D), cs = dot3(G.ng, T.ng);
                    const bool plane = nd * nd <= ((k_plane * k_plane) * fp2) * nn;
                    const bool normal = cs > 0.0f && cs * cs >= ((k_normal * k_normal) * nn) * dot3(T.ng, T.ng);
                    valid[k] = plane && normal;
                }
                n_valid += valid[k] ? 1 : 0;
            }
            count[(size_t)Y * ow + X] = n_valid;
            // 4. result
            Px r;
            if (n_valid == 4 || n_valid == 0) {
                const Px &a = color[tap[0]], &b = color[tap[1]], &c = color[tap[2]], &d = color[tap[3]];
                for (int ch = 0; ch < 4; ch++) r.c[ch] = (a.c[ch] * gx + b.c[ch] * fx) * gy + (c.c[ch] * gx + d.c[ch] * fx) * fy;
            } else {
                float S = 0.0f, C[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                for (int k = 0; k < 4; k++) {
                    if (!valid[k]) continue;
                    S = S + w[k];
                    for (int ch = 0; ch < 4; ch++) C[ch] = C[ch] + color[tap[k]].c[ch] * w[k];
                }
                for (int ch = 0; ch < 4; ch++) r.c[ch] = C[ch] / S;
            }
            out[(size_t)Y * ow + X] = r;
        }
    f = fopen(argv[6], "wb");
    if (!f || fwrite(out.data(), 16, n_out, f) != n_out || fwrite(count.data(), 4, n_out, f) != n_out) { fprintf(stderr, "upscale_guided_ref: cannot write %s\n", argv[6]); return 1; }
    fclose(f);
    return 0;
}
