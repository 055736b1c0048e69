// CPU restatement of the spatial variance estimate (hjr_estimate_variance), written from the specification in the header comment of
// henjou-renderer_amd/csrc/hjr_denoise.hip.h, not from the kernel: the GPU kernel must equal it bit for bit
// (tests/test_gpu_spatial_var.py), and the quality rehearsal of DESIGN.md §11.3 runs it on oracle frames.  Built by the tests with
// g++ -O2 -ffp-contract=off: fp32, every operation as written, fused only where fmaf says so.
//
//   spatial_var_ref W H has_vin in.bin out.bin [radius]
//     has_vin 1: in.bin carries an input variance; 0: every pixel is unknown
//     in.bin  float32: colour [H][W][4], albedo [H][W][4], normal [H][W][4], then with has_vin the variance [H][W]
//     out.bin float32: the variance [H][W]
//     radius  the window is (2 radius + 1)^2 taps (default 1, the library's 3 x 3; the rehearsal may pass 2)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// the portable exponential (Cephes expf: range reduction by ln 2 in two parts, degree-5 polynomial, scale by 2^n)
static float bits_to_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static float p_exp(float x)
{
    const float fn = floorf(fmaf(1.44269504088896341f, x, 0.5f));
    int n = (int)fn;
    float r = fmaf(fn, -0.693359375f, x);
    r = fmaf(fn, 2.12194440e-4f, r);
    const float z = r * r;
    float p = fmaf(1.9875691500e-4f, r, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f);
    p = fmaf(p, r, 4.1665795894e-2f);
    p = fmaf(p, r, 1.6666665459e-1f);
    p = fmaf(p, r, 5.0000001201e-1f);
    p = fmaf(p, z, r) + 1.0f;
    if (n > 127) { p = p * 1.70141183460469231732e38f; n -= 127; }
    if (n < -126) return 0.0f;
    return p * bits_to_float((uint32_t)(n + 127) << 23);
}
static float weight(float q, float phi) { return fminf(p_exp(fmaxf(-q / phi, -87.0f)), 1.0f); }
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct Px { float x, y, z, w; };

int main(int argc, char** argv)
{
    if (argc < 6) { fprintf(stderr, "usage: spatial_var_ref W H has_vin in.bin out.bin [radius]\n"); return 2; }
    const int W = atoi(argv[1]), H = atoi(argv[2]), has_vin = atoi(argv[3]), R = argc > 6 ? atoi(argv[6]) : 1;
    if (W <= 0 || H <= 0 || R < 1 || R > 8) { fprintf(stderr, "spatial_var_ref: bad arguments\n"); return 2; }
    const size_t n = (size_t)W * H;
    std::vector<Px> C(n), A(n), N(n);
    std::vector<float> V(n, 1e30f), out(n);
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(C.data(), 16, n, f) != n || fread(A.data(), 16, n, f) != n || fread(N.data(), 16, n, f) != n || (has_vin && fread(V.data(), 4, n, f) != n)) {
        fprintf(stderr, "spatial_var_ref: cannot read %s\n", argv[4]);
        return 1;
    }
    fclose(f);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t c = (size_t)y * W + x;
            const float K = fminf(fmaxf(V[c], 0.0f), 1e30f);
            if (K < 1e30f) { out[c] = V[c]; continue; } // a known variance passes through, bits unchanged
            const Px n0 = N[c], a0 = A[c];
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int dy = -R; dy <= R; dy++)
                for (int dx = -R; dx <= R; dx++) {
                    const size_t t = (size_t)clampi(y + dy, 0, H - 1) * W + clampi(x + dx, 0, W - 1);
                    const Px ct = C[t], nt = N[t], at = A[t];
                    const float lt = (ct.x + ct.y) + ct.z;
                    float ex = n0.x - nt.x, ey = n0.y - nt.y, ez = n0.z - nt.z;
                    const float wn = weight(ex * ex + ey * ey + ez * ez, 0.25f);
                    ex = a0.x - at.x; ey = a0.y - at.y; ez = a0.z - at.z;
                    const float wa = weight(ex * ex + ey * ey + ez * ez, 0.05f);
                    const float w = wn * wa;
                    s0 = s0 + w;
                    s1 = s1 + w * lt;
                    s2 = s2 + w * (lt * lt);
                }
            const float mu = s1 / s0;
            const float v = fmaxf(s2 / s0 - mu * mu, 0.0f);
            out[c] = (v < 1e30f) ? v : 1e30f;
        }
    f = fopen(argv[5], "wb");
    if (!f || fwrite(out.data(), 4, n, f) != n) { fprintf(stderr, "spatial_var_ref: cannot write %s\n", argv[5]); return 1; }
    fclose(f);
    return 0;
}
