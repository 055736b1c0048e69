// Denoise-mode replacement.  The reference runs the OptiX AI denoiser over (aov_color | guide albedo |
// guide normal) -> AOV_Output (renderer/denoiser.h:42-189, renderer/renderer.h:1093-1120, 1258-1270); that network is closed, so
// its pixels cannot be reproduced.  What is reproduced is the data flow of the three render modes (render_option.h:38-43):
//   Default            output = input                                   (blendFactor 1, denoiser.h:94-97)
//   Denoise            output = filter(color; albedo, normal), same size
//   DenoiseUpScale2X   rendered at (W/2, H/2) (renderer.h:1096-1099), filtered, then brought to W x H
// with an edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) guided by the same two AOVs, and a 2x bilinear
// upscale.  Build-defined, specified to the bit so that the test suite's CPU checker can restate it independently:
//   5 passes, tap distance 1, 2, 4, 8, 16; 5 x 5 taps with B3 weights h = (1/16, 1/4, 3/8, 1/4, 1/16), rows outer, clamped
//   to the frame; per tap  w = ((wc * wn) * wa) * (h[dy] * h[dx])  with  w? = min(p_exp(max(-q / phi, -87)), 1):
//     wn: q = |normal_c - normal_t|^2, phi 0.25;   wa: q = |albedo_c - albedo_t|^2, phi 0.05   (the two guide AOVs)
//     wc: passes 0 and 1: 1 (guides only: isolated fireflies are averaged away before the colour term can protect them);
//         passes 2, 3, 4: q = |colour_c - colour_t|^2 / (0.01 + s * s), s = (c.x + c.y) + c.z of the CURRENT centre colour,
//         phi = 1, 0.5, 0.25 (relative, so the tolerance follows the local radiance level);
//   |d|^2 = dx*dx + dy*dy + dz*dz; out.rgb = (sum of tap.rgb * w) / (sum of w), out.a = centre.a; fp32, no contraction,
//   p_exp = the portable exponential.  On the bundled scene against a 512 spp frame: RMSE 1.76 -> 0.15 at 4 spp, 0.32 -> 0.15
//   at 64 spp (light sources and background excluded).
// Streaming kernels, one lane per pixel: 75 float4 reads per pixel and pass (mostly L2 hits), bound by HBM/L2 bandwidth;
// < 1 % of a frame's render time.
//
// The VARIANCE-GUIDED variant (hjr_denoise_var, option "denoise_variance"): the spatial half of SVGF (Schied et al., HPG 2017) on the
// same guides.  The filter above has a floor (0.15 in the numbers above): its colour tolerance follows the radiance level, not how noisy
// the pixel still is, so its bias stays when the noise is gone.  Here the tolerance is the pixel's own standard deviation, from the
// variance AOV (hjr_render_var, DESIGN.md §4 rule 7), so the filter fades out as the frame converges.  Specified to the bit like the
// filter above; everything not named is as above (taps, clamping, h, wn, wa, n_phi, a_phi, the p_exp / max(., -87) / min(., 1) form,
// fp32 as written, no contraction):
//   two images ping-pong through the 5 passes (step 1, 2, 4, 8, 16): colour C (float4) and variance V (float, one per pixel); the input
//   variance is clamped once, as pass 0 reads it: V = fminf(fmaxf(V, 0.0f), 1e30f) (NaN and negative values act as 0);
//   per pass and centre pixel, the prefiltered variance: a 3 x 3 Gaussian of the pass's input V at distance 1 WHATEVER the step,
//     k3 = (0.25, 0.5, 0.25), rows outer, clamped to the frame:  gv = gv + V_t * (k3[j] * k3[i])  from +0.0f;  sd = sqrtf(gv);
//   colour weight, in ALL five passes:  l = (c.x + c.y) + c.z;  den = sigma_l * sd + eps;
//     wc = min(p_exp(max(-fabsf(l_c - l_t) / den, -87)), 1)   with sigma_l = 4 (the published value), eps = 1e-3;
//   w = ((wc * wn) * wa) * (h[dy] * h[dx]);   sums from +0.0f in tap order:  s = s + tap.rgb * w;  cum = cum + w;  sv = sv + V_t * (w * w);
//   C_out.rgb = s / cum, C_out.a = centre.a;   V_out = sv / (cum * cum)   (the variance of the weighted mean of independent taps).
// HJR_VARIANCE_UNKNOWN (1e30) needs no special case: sd is about 1e15, wc = 1, the filter weighs by the guides only, and no term
// overflows (V_t * w * w <= 1e30 * 0.02, 25 of them; cum >= the centre's 0.375 * 0.375).
// One more float per tap than the filter above (52 instead of 48 bytes) plus the 9 floats of the prefilter per pixel: 0.80 ms against
// 0.75 ms at 1080p.  On the bundled scene (96 x 64, box filling the frame, against a 16384 spp frame): RMSE 0.034 / 0.032 / 0.029 / 0.026
// at 16 / 64 / 256 / 1024 spp where the filter above stays at 0.059 / 0.057 / 0.056 / 0.056.
//
// The SPATIAL VARIANCE ESTIMATE (hjr_estimate_variance, option "denoise_variance_spatial"): what SVGF does while its history is short.  The
// variance AOV needs two full chunks of a pixel (rule 7), so a frame of at most 8 spp, and the first one-granule sample pass, carry
// HJR_VARIANCE_UNKNOWN everywhere and the variant above falls back to its guides.  This kernel fills such pixels with the guide-weighted
// second central moment of the luminance over the 3 x 3 neighbourhood and leaves every known variance as it is.  Specified to the bit;
// fp32 as written, no contraction, correctly rounded divide, p_exp = the portable exponential:
//   K = fminf(fmaxf(vin, 0.0f), 1e30f)          (NaN -> 0: the clamp hjr_atrous_kernel<true> applies to its input)
//   if K < 1e30f:  vout = vin as stored          (pass-through, the bits unchanged: negative values and NaN too, the filter clamps them)
//   else (HJR_VARIANCE_UNKNOWN and above, +Inf):
//     l = (c.x + c.y) + c.z of a tap's colour;  taps dy, dx in -1..1, rows outer, indices clamped to the frame, the centre included;
//     w = wn * wa  with the forms and constants of the filter above: q = |d|^2 of normal / albedo against the centre's, phi 0.25 / 0.05,
//         w? = min(p_exp(max(-q / phi, -87)), 1);
//     from +0.0f in tap order:  s0 = s0 + w;  s1 = s1 + w * l_t;  s2 = s2 + w * (l_t * l_t);
//     mu = s1 / s0;  v = fmaxf(s2 / s0 - mu * mu, 0.0f);
//     vout = (v < 1e30f) ? v : HJR_VARIANCE_UNKNOWN          (+Inf stays "unknown"; fmaxf turns a NaN difference into 0)
//   vin == NULL: every pixel is unknown.  vin is read at the centre only and by the lane that writes vout there, so vout == vin (in
//   place) is allowed.  s0 >= 1: the centre's weight is p_exp(-0) = 1.
// v estimates the variance of the pixel's written value r + g + b, the quantity rule 7 defines.  The window stays 3 x 3: a firefly
// inflates the estimate of every window that holds it, the colour weight opens there and the firefly spreads.
// One lane per pixel, 27 float4 and one float read, one float written; no LDS, no scratch.  0.055 ms at 1080p with every pixel unknown, 0.008 ms
// with every pixel known, next to the 0.86 ms of the five filter passes that follow (profiles/spatial_var.json).
//
// The GUIDED UPSCALE (hjr_upscale_guided, option "upscale_guided"): a joint-bilateral 2x upscale for DenoiseUpScale2X.  The a-trous passes
// are edge-avoiding so that colour does not cross a silhouette; the bilinear upscale below then crosses it again, and every geometric edge
// of the output is a two-pixel ramp between unrelated surfaces.  Here an output pixel keeps only those bilinear taps that lie on the surface
// its own centre ray hits, judged from two G-buffers of one camera (hjr_gbuffer_kernel at iw x ih and at ow x oh: the centre-ray expression
// u = (2 (px + 0.5) - W) / H sees the same view at both sizes).  Specified to the bit; fp32 as written, no contraction, correctly rounded
// divide.  Output pixel (X, Y) of ow x oh, low-resolution image iw x ih with ow / 2 == iw and oh / 2 == ih (integer division):
//   1. TAPS.  x0, y0, fx, fy, gx = 1 - fx, gy = 1 - fy and the clamped xa, xb, ya, yb exactly as hjr_upscale2x_kernel computes them.
//      Taps in order  a = (xa, ya), b = (xb, ya), c = (xa, yb), d = (xb, yb);  weights  w_a = gx * gy, w_b = fx * gy, w_c = gx * fy,
//      w_d = fx * fy  (products of quarters: exact).
//   2. RECORDS.  G = hi[Y * ow + X], T_k = lo[tap k], both hjr_gbuffer_px; cam: the one camera both G-buffers were traced from.
//   3. VALIDITY of tap k.  If G.prim == 0xffffffff (a miss): valid iff T_k.prim == 0xffffffff.  Otherwise valid iff T_k.prim != 0xffffffff,
//      T_k.inst == G.inst and both tests below hold (a NaN fails a comparison), with dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z:
//        D = T_k.pos - G.pos;  view = G.pos - cam.pos;  vv = dot(view, view);  fh = cam.f * (float)ih;  fp2 = (vv * 4) / (fh * fh)  (the squared
//        footprint of a LOW-resolution pixel at the point's distance);  nn = dot(G.ng, G.ng);  nd = dot(G.ng, D);  nt = T_k.ng;  cs = dot(G.ng, nt);
//        plane test:   nd * nd <= ((K_PLANE * K_PLANE) * fp2) * nn,  K_PLANE = 1;
//        normal test:  cs > 0  and  cs * cs >= ((K_NORMAL * K_NORMAL) * nn) * dot(nt, nt),  K_NORMAL = 0.9.
//   4. RESULT.  All four taps valid, or none: the bilinear expression of hjr_upscale2x_kernel as written, all four channels (such a pixel has
//      the BITS of the plain upscale).  Otherwise, from +0.0f, in tap order, over the valid taps only:  S = S + w_k;  C.c = C.c + tap.c * w_k
//      (c = x, y, z, w);  out.c = C.c / S.   S >= 0.0625: no division by zero.
// By construction: only pixels with at least one invalid tap change; memory is indexed by pixel coordinates only (no field of a caller-made
// record is an index, so hostile records cannot fault); a G-buffer in which no tap is ever valid gives the bilinear image.
// One lane per output pixel, 64 x 4 pixels per workgroup: 4 float4 colours, 4 low-resolution records and the lane's own record per lane (of
// a 48-byte record the 32 bytes prim .. ng are used), neighbouring lanes share their taps (L1 / L2 hits).  No LDS, no scratch.
// DESIGN.md §11.4 has the rehearsal and what was measured.
#pragma once
#include "hjr_math.hip.h"

#define HJR_ATROUS_PASSES 5
#define HJR_DENOISE_SIGMA_L 4.0f
#define HJR_DENOISE_VAR_EPS 1e-3f

#define HJR_DENOISE_N_PHI 0.25f
#define HJR_DENOISE_A_PHI 0.05f

// |a - b|^2 over x, y, z and the edge-stopping weight w? = min(p_exp(max(-q / phi, -87)), 1), as every rule above writes them
__device__ __forceinline__ float hjr_dist2(const float4& a, const float4& b)
{
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return dx * dx + dy * dy + dz * dz;
}
__device__ __forceinline__ float hjr_edge_weight(float q, float phi) { return fminf(p_exp(fmaxf(-q / phi, -87.0f)), 1.0f); }

// a variance as a pass of the variance-guided variant reads it: pass 0 (`clamp_in`) clamps its input
__device__ __forceinline__ float hjr_read_variance(const float* __restrict__ vin, size_t t, int clamp_in)
{
    const float v = vin[t];
    return clamp_in ? fminf(fmaxf(v, 0.0f), 1e30f) : v;
}

// One a-trous pass.  VAR false: the filter of the header's first block (vin, vout, clamp_in unused; c_phi 0: the colour term is off).
// VAR true: a pass of the variance-guided variant (c_phi unused; `clamp_in`: pass 0 clamps the variance as it reads it).
template <bool VAR>
__global__ void __launch_bounds__(256) hjr_atrous_kernel(const float4* __restrict__ in, const float* __restrict__ vin, const float4* __restrict__ normal,
                                                          const float4* __restrict__ albedo, float4* __restrict__ out, float* __restrict__ vout,
                                                          int W, int H, int step, int clamp_in, float c_phi)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const float hk[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
    const size_t c = (size_t)y * W + x;
    const float4 c0 = in[c], n0 = normal[c], a0 = albedo[c];
    const float l0 = (c0.x + c0.y) + c0.z;
    float den = 0.01f + l0 * l0; // VAR false: the relative colour tolerance
    if constexpr (VAR) {
        const float k3[3] = { 0.25f, 0.5f, 0.25f };
        float gv = 0.0f;
        for (int j = -1; j <= 1; j++) {
            const int yy = min(max(y + j, 0), H - 1);
            for (int i = -1; i <= 1; i++) {
                const int xx = min(max(x + i, 0), W - 1);
                gv = gv + hjr_read_variance(vin, (size_t)yy * W + xx, clamp_in) * (k3[j + 1] * k3[i + 1]);
            }
        }
        den = HJR_DENOISE_SIGMA_L * sqrtf(gv) + HJR_DENOISE_VAR_EPS;
    }
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, cum = 0.0f, sv = 0.0f;
    for (int j = -2; j <= 2; j++) {
        const int yy = min(max(y + j * step, 0), H - 1);
        for (int i = -2; i <= 2; i++) {
            const int xx = min(max(x + i * step, 0), W - 1);
            const size_t t = (size_t)yy * W + xx;
            const float4 ct = in[t], nt = normal[t], at = albedo[t];
            const float vt = VAR ? hjr_read_variance(vin, t, clamp_in) : 0.0f;
            float wc = 1.0f;
            if constexpr (VAR) wc = hjr_edge_weight(fabsf(l0 - ((ct.x + ct.y) + ct.z)), den);
            else if (c_phi > 0.0f) wc = hjr_edge_weight(hjr_dist2(c0, ct) / den, c_phi);
            const float wn = hjr_edge_weight(hjr_dist2(n0, nt), HJR_DENOISE_N_PHI);
            const float wa = hjr_edge_weight(hjr_dist2(a0, at), HJR_DENOISE_A_PHI);
            const float w = ((wc * wn) * wa) * (hk[j + 2] * hk[i + 2]);
            sx = sx + ct.x * w; sy = sy + ct.y * w; sz = sz + ct.z * w;
            cum = cum + w;
            if constexpr (VAR) sv = sv + vt * (w * w);
        }
    }
    out[c] = make_float4(sx / cum, sy / cum, sz / cum, c0.w);
    if constexpr (VAR) vout[c] = sv / (cum * cum);
}

// the spatial variance estimate (header above); vin NULL = every pixel unknown; vout may be vin (neither is __restrict__)
__global__ void __launch_bounds__(256) hjr_spatial_var_kernel(const float4* __restrict__ in, const float4* __restrict__ normal, const float4* __restrict__ albedo,
                                                               const float* vin, float* vout, int W, int H)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t c = (size_t)y * W + x;
    if (vin) {
        const float v0 = vin[c];
        if (fminf(fmaxf(v0, 0.0f), 1e30f) < 1e30f) { vout[c] = v0; return; }
    }
    const float4 n0 = normal[c], a0 = albedo[c];
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int j = -1; j <= 1; j++) {
        const int yy = min(max(y + j, 0), H - 1);
        for (int i = -1; i <= 1; i++) {
            const int xx = min(max(x + i, 0), W - 1);
            const size_t t = (size_t)yy * W + xx;
            const float4 ct = in[t], nt = normal[t], at = albedo[t];
            const float lt = (ct.x + ct.y) + ct.z;
            const float w = hjr_edge_weight(hjr_dist2(n0, nt), HJR_DENOISE_N_PHI) * hjr_edge_weight(hjr_dist2(a0, at), HJR_DENOISE_A_PHI);
            s0 = s0 + w; s1 = s1 + w * lt; s2 = s2 + w * (lt * lt);
        }
    }
    const float mu = s1 / s0;
    const float v = fmaxf(s2 / s0 - mu * mu, 0.0f);
    vout[c] = (v < 1e30f) ? v : 1e30f; // HJR_VARIANCE_UNKNOWN
}

// The taps of output pixel (X, Y) of a 2x upscale, pixel centres: source coordinate (X + 0.5) / 2 - 0.5, i.e. weights 0.75 / 0.25 towards
// the nearer texel (fx, fy: the weights of the second tap column / row), indices clamped to the source frame; a, b, c, d: the taps' pixel indices
struct Upscale2xTaps {
    float fx, fy;
    size_t a, b, c, d;
};
__device__ __forceinline__ Upscale2xTaps hjr_upscale2x_taps(int X, int Y, int iw, int ih)
{
    const int x0 = (X & 1) ? (X >> 1) : (X >> 1) - 1, y0 = (Y & 1) ? (Y >> 1) : (Y >> 1) - 1;
    const int xa = min(max(x0, 0), iw - 1), xb = min(max(x0 + 1, 0), iw - 1);
    const int ya = min(max(y0, 0), ih - 1), yb = min(max(y0 + 1, 0), ih - 1);
    Upscale2xTaps t;
    t.fx = (X & 1) ? 0.25f : 0.75f; t.fy = (Y & 1) ? 0.25f : 0.75f;
    t.a = (size_t)ya * iw + xa; t.b = (size_t)ya * iw + xb; t.c = (size_t)yb * iw + xa; t.d = (size_t)yb * iw + xb;
    return t;
}
// out = (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy per channel
__device__ __forceinline__ float4 hjr_bilinear(const float4& a, const float4& b, const float4& c, const float4& d, float fx, float fy)
{
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    float4 r;
    r.x = (a.x * gx + b.x * fx) * gy + (c.x * gx + d.x * fx) * fy;
    r.y = (a.y * gx + b.y * fx) * gy + (c.y * gx + d.y * fx) * fy;
    r.z = (a.z * gx + b.z * fx) * gy + (c.z * gx + d.z * fx) * fy;
    r.w = (a.w * gx + b.w * fx) * gy + (c.w * gx + d.w * fx) * fy;
    return r;
}

// 2x bilinear upscale
__global__ void __launch_bounds__(256) hjr_upscale2x_kernel(const float4* __restrict__ in, float4* __restrict__ out, int iw, int ih, int ow, int oh)
{
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (X >= ow || Y >= oh) return;
    const Upscale2xTaps t = hjr_upscale2x_taps(X, Y, iw, ih);
    out[(size_t)Y * ow + X] = hjr_bilinear(in[t.a], in[t.b], in[t.c], in[t.d], t.fx, t.fy);
}

// the guided 2x upscale (header above): is the low-resolution record T on the surface of the output pixel's record G?
#define HJR_UPSCALE_K_PLANE 1.0f
#define HJR_UPSCALE_K_NORMAL 0.9f
__device__ __forceinline__ bool hjr_upscale_tap_valid(const hjr_gbuffer_px& G, const hjr_gbuffer_px& T, float lim_plane, float lim_normal)
{
    if (G.prim == 0xffffffffu) return T.prim == 0xffffffffu;
    if (T.prim == 0xffffffffu || T.inst != G.inst) return false;
    const float dx = T.pos[0] - G.pos[0], dy = T.pos[1] - G.pos[1], dz = T.pos[2] - G.pos[2];
    const float nd = (G.ng[0] * dx + G.ng[1] * dy) + G.ng[2] * dz;
    const float cs = (G.ng[0] * T.ng[0] + G.ng[1] * T.ng[1]) + G.ng[2] * T.ng[2];
    const float tt = (T.ng[0] * T.ng[0] + T.ng[1] * T.ng[1]) + T.ng[2] * T.ng[2];
    return nd * nd <= lim_plane && cs > 0.0f && cs * cs >= lim_normal * tt;
}

__global__ void __launch_bounds__(256) hjr_upscale_guided_kernel(const float4* __restrict__ in, const hjr_gbuffer_px* __restrict__ lo, const hjr_gbuffer_px* __restrict__ hi,
                                                                  float4* __restrict__ out, const hjr_camera cam, int iw, int ih, int ow, int oh)
{
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (X >= ow || Y >= oh) return;
    const Upscale2xTaps t = hjr_upscale2x_taps(X, Y, iw, ih);
    const float4 a = in[t.a], b = in[t.b], c = in[t.c], d = in[t.d];
    const hjr_gbuffer_px G = hi[(size_t)Y * ow + X];
    const float vx = G.pos[0] - cam.pos[0], vy = G.pos[1] - cam.pos[1], vz = G.pos[2] - cam.pos[2];
    const float vv = (vx * vx + vy * vy) + vz * vz;
    const float fh = cam.f * (float)ih;
    const float fp2 = (vv * 4.0f) / (fh * fh);
    const float nn = (G.ng[0] * G.ng[0] + G.ng[1] * G.ng[1]) + G.ng[2] * G.ng[2];
    const float lim_plane = ((HJR_UPSCALE_K_PLANE * HJR_UPSCALE_K_PLANE) * fp2) * nn;
    const float lim_normal = (HJR_UPSCALE_K_NORMAL * HJR_UPSCALE_K_NORMAL) * nn;
    const bool va = hjr_upscale_tap_valid(G, lo[t.a], lim_plane, lim_normal), vb = hjr_upscale_tap_valid(G, lo[t.b], lim_plane, lim_normal);
    const bool vc = hjr_upscale_tap_valid(G, lo[t.c], lim_plane, lim_normal), vd = hjr_upscale_tap_valid(G, lo[t.d], lim_plane, lim_normal);
    const int n_valid = (int)va + (int)vb + (int)vc + (int)vd;
    float4 r;
    if (n_valid == 4 || n_valid == 0) r = hjr_bilinear(a, b, c, d, t.fx, t.fy);
    else {
        const float gx = 1.0f - t.fx, gy = 1.0f - t.fy;
        const float wa = gx * gy, wb = t.fx * gy, wc = gx * t.fy, wd = t.fx * t.fy;
        float S = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f, cw = 0.0f;
        if (va) { S = S + wa; cx = cx + a.x * wa; cy = cy + a.y * wa; cz = cz + a.z * wa; cw = cw + a.w * wa; }
        if (vb) { S = S + wb; cx = cx + b.x * wb; cy = cy + b.y * wb; cz = cz + b.z * wb; cw = cw + b.w * wb; }
        if (vc) { S = S + wc; cx = cx + c.x * wc; cy = cy + c.y * wc; cz = cz + c.z * wc; cw = cw + c.w * wc; }
        if (vd) { S = S + wd; cx = cx + d.x * wd; cy = cy + d.y * wd; cz = cz + d.z * wd; cw = cw + d.w * wd; }
        r = make_float4(cx / S, cy / S, cz / S, cw / S);
    }
    out[(size_t)Y * ow + X] = r;
}
