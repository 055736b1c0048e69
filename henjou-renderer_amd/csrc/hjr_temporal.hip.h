// Temporal accumulation with reprojection for the Denoise modes: the temporal half of SVGF (Schied et al., HPG 2017) in front of the
// variance-guided a-trous filter (hjr_denoise.hip.h).  Two kernels, both outside the render kernels (no render kernel knows about them):
//   hjr_gbuffer_kernel<WIDTH, COV>   first-hit record of every pixel's centre ray, by the stand-alone traversal the tile classifier uses;
//   hjr_temporal_kernel<COV, MOM>  one lane per pixel: reprojects the pixel's surface point into the previous frame, gathers the previous
//                               frame's accumulated colour / variance / history length with four validated bilinear taps and blends.
//   hjr_temporal_resp_kernel<COV, MOM>  the same with the windowed change test of section RESPONSE: a workgroup per 16 x 16 pixels.
//   hjr_temporal_prior_kernel<COV>      the gather alone, ahead of the frame's render: section PRIOR.
// Included by hjr_post.hip only: correctly rounded divide, no contraction, denormals on.  Specified to the bit, so that the test suite's
// CPU checker (tests/native/temporal_ref.cpp) restates it independently.  fp32 throughout, every operation as written, left to right:
//   dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z ;   cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x) ;
//   a 3 x 4 row-major transform M (12 floats, as hjr_set_transforms) applied to a point:  xf(M, p).i = ((M[4i] * p.x + M[4i+1] * p.y) + M[4i+2] * p.z) + M[4i+3],
//   its linear part applied to a vector:  lin(M, d).i = (M[4i] * d.x + M[4i+1] * d.y) + M[4i+2] * d.z ;   finite(x) = fabsf(x) <= FLT_MAX.
//
// G-BUFFER.  Pixel (px, py), W x H, exactly the tile classifier's ray:  u = (2 (px + 0.5) - W) / H,  v = (2 (py + 0.5) - H) / H,
//   d = normalize(dir * f + right * u + up * v), origin cam.pos, tmin 0.001, tmax 1e16; traverse<ANY = false> against the frame data read
//   from memory.  A hit with row k of the leaf-ordered triangle array (v0, v1, v2 world space) gives the record
//     prim, inst = tri_inst[prim], t, b1, b2,  pos = v0 * (1 - b1 - b2) + v1 * b1 + v2 * b2  (hit_program's expression: per component
//     (v0.c * w0 + v1.c * b1) + v2.c * b2 with w0 = (1 - b1) - b2),  ng = cross(v1 - v0, v2 - v0)  (not normalised),  pad = 0.
//   A miss (or a prim id outside the triangle table) is prim = 0xffffffff and every other field 0.
//
// ACCUMULATION.  Pixel (x, y) of the current frame, G = cur.gbuffer[y W + x]; cur / prev: hjr_temporal_frame.  RESTART means
//   out = cur.color, var = cur.variance, h = 1  (all three copied as stored).
//   1. RESTART if there is no previous frame, or G.prim == 0xffffffff, or G.prim >= n_triangles, or G.inst >= n_instances.
//   2. p_obj = xf(Minv_cur[G.inst], G.pos);  p_prev = xf(M_prev[G.inst], p_obj);  w = p_prev - prev.camera.pos;
//      a = prev.camera.dir * prev.camera.f,  b = prev.camera.right,  c = prev.camera.up  (right is not normalised: a full 3 x 3 solve);
//      bc = cross(b, c);  det = dot(a, bc);  s = dot(w, bc) / det;  su = dot(a, cross(w, c)) / det;  sv = dot(a, cross(b, w)) / det;
//      u = su / s;  v = sv / s;   RESTART unless det != 0 and s > 0 and finite(s), finite(u), finite(v);
//      xp = (u * H + W) * 0.5 - 0.5;  yp = (v * H + H) * 0.5 - 0.5;   RESTART unless xp >= -1 and xp < W and yp >= -1 and yp < H  (float compares);
//      fx = floorf(xp), fy = floorf(yp);  x0 = (int)fx, y0 = (int)fy;  tx = xp - fx, ty = yp - fy.
//   3. Taps k = 0..3 at (x0 + (k & 1), y0 + (k >> 1)), weights  w0 = (1 - tx) * (1 - ty), w1 = tx * (1 - ty), w2 = (1 - tx) * ty, w3 = tx * ty.
//      Tap k with record T = prev.gbuffer[tap] is VALID iff it lies inside the image, T.prim != 0xffffffff, T.prim < n_triangles,
//      T.inst == G.inst, and with
//        e = xf(Minv_prev[T.inst], T.pos) - p_obj;  D = lin(M_cur[G.inst], e);  view = G.pos - cur.camera.pos;  ng = G.ng;
//        vv = dot(view, view);  fh = cur.camera.f * H;  fp2 = (vv * 4) / (fh * fh);  nn = dot(ng, ng);  nd = dot(ng, D);  nv = dot(ng, view);
//      both   nd * nd <= ((K_PLANE * K_PLANE) * fp2) * nn   and   dot(D, D) * (nv * nv) <= (((K_DIST * K_DIST) * fp2) * nn) * vv
//      hold (a NaN fails a comparison).  fp2 is the squared footprint of a pixel at the point's distance; the first test is the distance
//      from the current tangent plane, the second the distance in the plane scaled by the cosine of the view angle.
//   4. In tap order over the valid taps, all sums from +0.0f:  S = S + w_k;  C.c = C.c + prev.color[tap].c * w_k (c = r, g, b);
//      with pv = prev.variance[tap]:  unknown |= !(pv < HJR_VARIANCE_UNKNOWN)  (NaN included);  V = V + fmaxf(pv, 0) * w_k;
//      Hs = Hs + prev.history[tap] * w_k.   RESTART unless S > 0.   c_prev = C / S,  v_prev = V / S,  h_prev = Hs / S  (one divide each);
//      h = fminf(fmaxf(h_prev + 1, 1), 64);   al = fmaxf(1 / h, HJR_TEMPORAL_ALPHA);
//      out.c = c_prev.c + (cur.c - c_prev.c) * al,  out.a = cur.a;
//      cv = cur.variance;  unknown |= !(cv < HJR_VARIANCE_UNKNOWN);  om = 1 - al;
//      var = unknown ? HJR_VARIANCE_UNKNOWN : (om * om) * v_prev + (al * al) * fmaxf(cv, 0)     (fmaxf(NaN, 0) = 0 never reaches the sum).
//   The variance is that of a convex combination of independent estimates (frames are independent: the RNG index is frame * spp + s), which
//   is why it is propagated and not estimated from temporal moments (section TEMPORAL MOMENTS below adds that estimate, opt-in, for frames
//   whose own variance is unknown).  K_PLANE = 1, K_DIST = 3: "a tap is at most one pixel from the exact
//   point" (DESIGN.md §11 has what was measured).
// Hostile input: every table index (instance of the current record and of each tap) is range-checked before it is used, no tap outside the
// image is read, and float -> int conversion happens only after the float range check; nothing else indexes memory.
//
// COVERAGE G-BUFFER (hjr_gbuffer_kernel<WIDTH, true>, side n = 2, 3 or 4).  The centre ray and its record are exactly the
//   G-BUFFER's above; only `pad` differs.  After the centre ray, n * n sub-pixel rays, no RNG: sub-ray (i, j), i, j = 0..n-1, j the outer
//   loop:  ox = ((float)i + 0.5f) / (float)n,  oy = ((float)j + 0.5f) / (float)n,  u = (2 (px + ox) - W) / H,  v = (2 (py + oy) - H) / H,
//   direction, origin, tmin and tmax by the centre ray's expression.  A sub-ray is ON THE CENTRE'S SURFACE iff
//     both rays miss (a prim id outside the triangle table is a miss), or
//     both hit, tri_inst[prim_sub] == G.inst, the material words agree (word 15 of the prims' tri_shade rows: what separates an emitter
//     quad from the coplanar ceiling of the same mesh), and   nd * nd <= ((K_PLANE * K_PLANE) * fp2) * nn   with
//       D = pos_sub - G.pos  (pos_sub by the record's own `pos` expression),  nd = dot(G.ng, D),  nn = dot(G.ng, G.ng),
//       view = G.pos - cam.pos,  vv = dot(view, view),  fh = cam.f * H,  fp2 = (vv * 4) / (fh * fh)   (dot as above; a NaN fails).
//   pad = same | (n * n) << 8, `same` the number of sub-rays on the centre's surface.  A miss record carries its counts too (a sky pixel
//   that partly covers geometry is known); every other field of a miss record stays 0.  hjr_gbuffer_kernel<WIDTH, false> writes pad = 0.
//
// COVERAGE-AWARE ACCUMULATION (hjr_temporal_kernel<true>: the ACCUMULATION above with two more inputs, prev.coverage and cur.coverage, the
//   `coverage` fields of the two hjr_temporal_frame (and of the two TemporalSide); with both 0 it is the rule above bit for bit, and that
//   case runs hjr_temporal_kernel<false>).
//   A record R of a side whose coverage != 0 is MIXED iff  total = (R.pad >> 8) & 0xff  is above 0 and  (R.pad & 0xff) < total;  a record of a
//   side whose coverage == 0 is never mixed and its pad is not looked at.  pad is only ever compared, never used as an index.
//   3'. G not mixed: a tap whose record T (of prev) is mixed is INVALID; everything else is unchanged.
//   2'. G mixed: after step 2's xp, yp (and its RESTART tests):  xr = floorf(xp + 0.5f),  yr = floorf(yp + 0.5f);
//       RESTART unless  fabsf(xp - xr) <= HJR_TEMPORAL_SNAP  and  fabsf(yp - yr) <= HJR_TEMPORAL_SNAP  (a NaN fails the comparison).
//       Otherwise the only tap is (xr, yr) (converted to int after step 2's range test, so within [-1, W] x [-1, H]) with weight exactly
//       1.0f, subject to rule 3's validity tests (inside the image, prim, instance, plane, distance) and, if prev.coverage != 0, to
//       T.pad == G.pad (all 32 bits).  Step 4 proceeds with that one tap: S = 1, and the divides are still performed.
//   In words: a mixed pixel keeps its history only from the pixel it coincides with, and otherwise restarts; a full pixel never taps a mixed
//   one.  A static sequence still accumulates everywhere: the reprojection lands on the centre up to rounding.
//
// TEMPORAL MOMENTS (hjr_temporal_kernel<COV, true>: the ACCUMULATION above, with or without the coverage rules, with one more input,
//   prev.moments (a field of the device-side TemporalSide; the public entry points take it as their prev_moments argument, it is no field
//   of hjr_temporal_frame), and one more output, both float2 (m1, m2) per pixel: the accumulated first and second moment of the luminance
//     l = (cur.r + cur.g) + cur.b     of the current frame's colour as the kernel reads it.   DESIGN.md §11.7.)
//   RESTART (every case above): additionally  m1 = l,  m2 = l * l.   Colour, variance and h are the ones above.
//   4. per valid tap, in tap order, both sums from +0.0f, pm = prev.moments[tap]:   M1 = M1 + pm.x * w_k;   M2 = M2 + pm.y * w_k.
//      After S > 0:   m1p = M1 / S,  m2p = M2 / S  (one divide each);   m1 = m1p + (l - m1p) * al,   m2 = m2p + (l * l - m2p) * al
//      (al the colour's blend factor).   If  h >= HJR_TEMPORAL_MOMENTS_MIN  the variance of step 4 is replaced by
//        k = fmaxf(1 / h, HJR_TEMPORAL_ALPHA / (2 - HJR_TEMPORAL_ALPHA));   d = m2 - m1 * m1;
//        var = finite(d) ? fmaxf(d, 0) * (k / (1 - k)) : HJR_VARIANCE_UNKNOWN;   a var that is not below HJR_VARIANCE_UNKNOWN is written as
//        HJR_VARIANCE_UNKNOWN.   Otherwise (h < HJR_TEMPORAL_MOMENTS_MIN) the variance is step 4's, "unknown" included.
//   k is the sum of the squared blend weights of the frames in the accumulated colour: 1 / h while the blend is a plain mean, with limit
//   alpha / (2 - alpha) once al stays at alpha.  1 / (1 - k) unbiases the weighted sample variance m2 - m1 * m1 of one frame's luminance, and
//   the factor k turns the variance of one frame's value into that of the accumulated colour, which is what rule 7 and the filter expect.
//   With a fractional h after bilinear mixing the weights are not exactly those, so k is approximate there.
//   Rules 2' / 3' choose the taps as above; the moments ride on whichever taps are chosen.  Moments are only ever multiplied, added and
//   compared: NaN, Inf and values whose square overflows end in HJR_VARIANCE_UNKNOWN or a finite variance, and index nothing.
//
// RESPONSE (hjr_temporal_resp_kernel<COV, MOM>: the ACCUMULATION above, with or without the coverage rules and the moments, with one more
//   output, lambda per pixel (float, [H][W]).  DESIGN.md §11.8.)  Reprojection follows surfaces, not illumination; this section lets the
//   history give way where the window mean of the current luminance has left that of the reprojected history.
//   Steps 1 to 4 are unchanged up to c_prev, v_prev, h_prev (with 2' / 3', and the moments' m1p, m2p).  A pixel is CARRIED iff it did not
//   RESTART.  For a pixel q:   lc_q = (cur.r + cur.g) + cur.b  of q's current colour;   for a carried q,  lp_q = (c_prev.r + c_prev.g) + c_prev.b
//   of q's own c_prev.
//   For a carried pixel p with record G_p the window is the (2 R + 1)^2 pixels (x + dx, y + dy), dy the outer loop and dx the inner one, both
//   from -R to R.  A pixel q of it is a MEMBER iff it lies in the image, G_q.prim != 0xffffffff and G_q.prim < n_triangles,
//   G_q.inst == G_p.inst, and q is carried (p is a member of its own window).  In window order over the members, all sums from +0.0f, n the
//   number of members:   Sd = Sd + (lc_q - lp_q);   Sc = Sc + lc_q;   Sc2 = Sc2 + lc_q * lc_q.   Then
//     nf = (float)n;  mu_d = Sd / nf;  mu_c = Sc / nf;  var_c = fmaxf(Sc2 / nf - mu_c * mu_c, 0);  se = sqrtf(var_c / nf) + EPS;
//     t = fabsf(mu_d) / se;   lambda = (n >= NMIN) ? fminf(fmaxf((t - T0) / (T1 - T0), 0), 1) : 0      (a NaN t gives 0 through fmaxf).
//   The blend of step 4 and of the moments uses  al' = fmaxf(al, lambda)  wherever they use al: the colour, om = 1 - al', the propagated
//   variance, m1 and m2.  The history length becomes  h = (lambda > 0) ? fminf(h, 1 / al') : h  (after al was taken from the unchanged h),
//   and that h is the one written and the one the moments' test  h >= HJR_TEMPORAL_MOMENTS_MIN  and their k see.
//   RESTART pixels write lambda = 0 and everything else as above.
//   R, T0, T1, NMIN, EPS are HJR_TEMPORAL_RESP_R (2), _T0 (3), _T1 (6), _NMIN (5), _EPS (1e-3f) of include/henjou_hip.h.
//   The difference of the means is judged against the spread of the current frame alone: sqrt(var_c / n) is the standard error of the
//   window mean of one frame, so t counts standard errors, and the history's own (smaller) noise is left out.  With lambda = 0 in a pixel
//   its outputs are the bits of the kernel without this section: fmaxf(al, 0) = al exactly, and h is untouched.
//   Luminances are only added, multiplied, divided and compared, and the window is addressed by integer pixel offsets inside the image:
//   NaN, Inf and overflowing squares end in a lambda in [0, 1] and index nothing.
//
// PRIOR (hjr_temporal_prior_kernel<COV>: what the history will contribute to a pixel of the frame that is about to be rendered, before any
//   of its colour exists; adaptive sampling's rule 11 reads it, csrc/hjr_aux.hip.h and DESIGN.md §4 rule 11.)  One float4 (lp, vp, al, 0) per
//   pixel, [H][W].  Steps 1 to 4 of ACCUMULATION (with 2' / 3' when a side carries coverage) run unchanged up to c_prev, v_prev, h_prev and
//   the taps' `unknown`; cur.color and cur.variance are never read (cur is the G-buffer, camera and transforms of the coming frame).
//   A CARRIED pixel (one that did not RESTART) whose taps' `unknown` is false writes
//     h = fminf(fmaxf(h_prev + 1, 1), 64);   al = fmaxf(1 / h, HJR_TEMPORAL_ALPHA);   lp = (c_prev.r + c_prev.g) + c_prev.b;   vp = v_prev
//   (h and al are step 4's, so al is the factor the accumulation will blend this pixel's colour with).  Every other pixel (a RESTART of any
//   kind, no previous frame, an unknown variance in a tap) writes (0, 0, 1, 0): al = 1 says "the current frame stands alone".
//   Neither section RESPONSE's lambda nor the TEMPORAL MOMENTS enter: both need the current frame's colour, which does not exist yet.  With
//   those options on the accumulation still applies them, and the prior is then the blend they would leave with lambda = 0 and the
//   propagated variance: a limit of the prior, not of the accumulation.
//   c_prev, v_prev and h_prev are only added, divided and compared: a NaN h_prev gives al = 1 through fmaxf, a NaN lp or vp is written as it is
//   (rule 11 falls back to rule 6 on a NaN) and nothing indexes memory.
#pragma once
#include "hjr_traverse.hip.h" // TileStack: the classifier's stacks

#define HJR_TEMPORAL_K_PLANE 1.0f
#define HJR_TEMPORAL_K_DIST 3.0f
#define HJR_TEMPORAL_H_MAX 64.0f

struct GbufArgs {
    const float4* nodes;
    const float4* tri_geom;
    const uint32_t* tri_inst;
    const uint32_t* tri_shade; // COV: the shading rows as words: word 15 of a row is the material id
    uint32_t n_tris, width, height, tiles_x, n_tiles;
    uint32_t side;             // COV: 2, 3 or 4
    hjr_camera cam;
    hjr_gbuffer_px* out;
};

HD float t_dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// One wave per 8 x 8 tile, grid-stride over the tiles; 64 * stack_depth * 4 bytes of dynamic LDS (the classifier's stacks).  Per pixel the
// centre ray (iteration 0) and, COV, the n * n sub-pixel rays (iterations 1 .. n * n) go through one traversal call site, every lane of a
// wave runs all iterations, and what is carried from the centre to the sub-rays are scalars (no per-lane array).
template <int WIDTH, bool COV>
__global__ void __launch_bounds__(64) hjr_gbuffer_kernel(const GbufArgs A)
{
    TileStack stack = hjr_tile_stack();
    const uint32_t n = COV ? A.side : 1u, n_rays = COV ? n * n : 0u;
    for (uint32_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        uint32_t tx, ty;
        hjr_tile_xy(tile, A.tiles_x, &tx, &ty);
        const uint32_t px = tx * HJR_TILE + (threadIdx.x & 7u), py = ty * HJR_TILE + (threadIdx.x >> 3);
        if (px >= A.width || py >= A.height) continue;
        const float W = (float)A.width, H = (float)A.height;
        const f3 cd = V(A.cam.dir[0], A.cam.dir[1], A.cam.dir[2]), cu = V(A.cam.up[0], A.cam.up[1], A.cam.up[2]);
        const f3 cr = V(A.cam.right[0], A.cam.right[1], A.cam.right[2]), cp = V(A.cam.pos[0], A.cam.pos[1], A.cam.pos[2]);
        hjr_gbuffer_px r;
        r.prim = 0xffffffffu; r.inst = 0u; r.t = r.b1 = r.b2 = 0.0f; r.pad = 0u;
        for (int k = 0; k < 3; k++) r.pos[k] = r.ng[k] = 0.0f;
        uint32_t c_mat = 0u, same = 0u;
        float lim = 0.0f;
        for (uint32_t it = 0; it <= n_rays; it++) {
            const uint32_t s = it ? it - 1u : 0u;
            const float ox = it ? ((float)(s % n) + 0.5f) / (float)n : 0.5f, oy = it ? ((float)(s / n) + 0.5f) / (float)n : 0.5f;
            const float u = (2.0f * ((float)px + ox) - W) / H, v = (2.0f * ((float)py + oy) - H) / H;
            const f3 d = normalize(cd * A.cam.f + cr * u + cu * v);
            Hit h;
            Counters cnt; cnt.box = cnt.tri = 0;
            const bool hit = traverse<false, false, WIDTH, 64, TileStack>(A.nodes, A.tri_geom, cp, d, 0.001f, 1e16f, h, stack, cnt) && h.prim < A.n_tris;
            f3 pos = V1(0.0f), ng = V1(0.0f);
            uint32_t inst = 0u, mat = 0u;
            if (hit) {
                const float4* g = A.tri_geom + (size_t)h.k * HJR_TRI_F4;
                const float4 g0 = g[0], g1 = g[1], g2 = g[2];
                const f3 v0 = V(g0.x, g0.y, g0.z), v1 = V(g0.w, g1.x, g1.y), v2 = V(g1.z, g1.w, g2.x);
                const float w0 = 1.0f - h.b1 - h.b2;
                pos = v0 * w0 + v1 * h.b1 + v2 * h.b2;
                ng = cross(v1 - v0, v2 - v0);
                inst = A.tri_inst[h.prim];
                if constexpr (COV) mat = A.tri_shade[(size_t)h.prim * (HJR_SHADE_F4 * 4) + 15u];
            }
            if (it == 0u) {
                if (hit) {
                    r.prim = h.prim; r.inst = inst;
                    r.t = h.t; r.b1 = h.b1; r.b2 = h.b2;
                    r.pos[0] = pos.x; r.pos[1] = pos.y; r.pos[2] = pos.z;
                    r.ng[0] = ng.x; r.ng[1] = ng.y; r.ng[2] = ng.z;
                    if constexpr (COV) {
                        c_mat = mat;
                        const f3 view = pos - cp;
                        const float vv = t_dot(view, view), fh = A.cam.f * H;
                        const float fp2 = (vv * 4.0f) / (fh * fh), nn = t_dot(ng, ng);
                        lim = ((HJR_TEMPORAL_K_PLANE * HJR_TEMPORAL_K_PLANE) * fp2) * nn;
                    }
                }
            } else if (r.prim == 0xffffffffu) {
                same += hit ? 0u : 1u;
            } else if (hit && inst == r.inst && mat == c_mat) {
                const float nd = t_dot(V(r.ng[0], r.ng[1], r.ng[2]), pos - V(r.pos[0], r.pos[1], r.pos[2]));
                same += nd * nd <= lim ? 1u : 0u;
            }
        }
        if constexpr (COV) r.pad = same | (n_rays << 8);
        A.out[(size_t)py * A.width + px] = r;
    }
}

// device view of one frame: a hjr_temporal_frame and, for prev, the entry points' prev_moments
struct TemporalSide {
    hjr_camera cam;
    const float* m;             // n_instances x 12
    const float* inv;           // n_instances x 12
    const hjr_gbuffer_px* gbuf;
    const float4* color;
    const float* variance;
    const float* history;       // prev only
    const float2* moments;      // MOM, prev only
    uint32_t coverage;          // COV: hjr_temporal_frame.coverage
};
// what a launch writes; the two optional images choose the kernel (hjr_post.hip: temporal_launch)
struct TemporalOut {
    float4* color;
    float* variance;
    float* history;
    float2* moments;            // MOM
    float* response;            // hjr_temporal_resp_kernel: lambda
};
struct TemporalArgs {
    TemporalSide cur, prev;     // prev is all zero unless have_prev (cur first: with prev first hjr_temporal_resp_kernel<false, true> keeps
                                // 10 SGPRs in VGPR lanes for 8)
    TemporalOut out;
    uint32_t have_prev, width, height, n_instances, n_tris;
};

HD f3 t_xf(const float* __restrict__ m, f3 p)
{
    return V(((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3], ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7], ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11]);
}
HD f3 t_lin(const float* __restrict__ m, f3 d)
{
    return V((m[0] * d.x + m[1] * d.y) + m[2] * d.z, (m[4] * d.x + m[5] * d.y) + m[6] * d.z, (m[8] * d.x + m[9] * d.y) + m[10] * d.z);
}
HD bool t_finite(float x) { return fabsf(x) <= HJ_FLT_MAX; }
HD bool t_mixed(uint32_t pad) { const uint32_t total = (pad >> 8) & 0xffu; return total > 0u && (pad & 0xffu) < total; }

// COV: the coverage-aware accumulation (rules 2' and 3' of the header comment), launched only when a side carries coverage.  Its four
// expressions (g_mixed, the snap tap, n_taps, the pad test of a tap) are constants in the plain instantiation and fold away there.
// MOM: the temporal luminance moments (section TEMPORAL MOMENTS of the header comment): one float2 load per valid tap, one float2 store
// per pixel; every line of it sits under `if constexpr (MOM)`, so the MOM = false instantiations are the code they were without it.

// what steps 1 to 4 gather of the previous frame for one pixel: c_prev, v_prev, h_prev (and m1p, m2p) and the taps' "unknown"
struct TemporalPrev {
    float cx, cy, cz, v, h;
    bool unknown;
    float m1, m2;  // MOM
    uint32_t inst; // the pixel's instance, < n_instances
};

// Steps 1 to 4 of ACCUMULATION (with 2' / 3' and the moments' sums) for the pixel whose record is G, up to the divides by S: a carried
// pixel calls carried(P) at the place step 4 blends, a RESTART calls nothing.  Shared by hjr_temporal_kernel and hjr_temporal_resp_kernel.
// A callback and the argument block by value, not a returned flag and a reference: by reference the plain-G-buffer response kernels keep
// 12 and 10 SGPRs in VGPR lanes for 4 and 8, and every kernel is 6 to 48 instructions longer (profiles/temporal_fold_kernel_resources.txt).
template <bool COV, bool MOM, typename Carried>
__device__ __forceinline__ void hjr_temporal_gather(const TemporalArgs A, const size_t pix, Carried carried)
{
    const hjr_gbuffer_px G = A.cur.gbuf[pix];
    if (A.have_prev && G.prim != 0xffffffffu && G.prim < A.n_tris && G.inst < A.n_instances) {
        const float W = (float)A.width, H = (float)A.height;
        const f3 gpos = V(G.pos[0], G.pos[1], G.pos[2]);
        const f3 p_obj = t_xf(A.cur.inv + (size_t)G.inst * 12u, gpos);
        const f3 p_prev = t_xf(A.prev.m + (size_t)G.inst * 12u, p_obj);
        const f3 w = p_prev - V(A.prev.cam.pos[0], A.prev.cam.pos[1], A.prev.cam.pos[2]);
        const f3 a = V(A.prev.cam.dir[0] * A.prev.cam.f, A.prev.cam.dir[1] * A.prev.cam.f, A.prev.cam.dir[2] * A.prev.cam.f);
        const f3 b = V(A.prev.cam.right[0], A.prev.cam.right[1], A.prev.cam.right[2]), c = V(A.prev.cam.up[0], A.prev.cam.up[1], A.prev.cam.up[2]);
        const f3 bc = cross(b, c);
        const float det = t_dot(a, bc);
        const float s = t_dot(w, bc) / det, su = t_dot(a, cross(w, c)) / det, sv = t_dot(a, cross(b, w)) / det;
        const float u = su / s, v = sv / s;
        const float xp = (u * H + W) * 0.5f - 0.5f, yp = (v * H + H) * 0.5f - 0.5f;
        if (det != 0.0f && s > 0.0f && t_finite(s) && t_finite(u) && t_finite(v) && xp >= -1.0f && xp < W && yp >= -1.0f && yp < H) {
            const bool g_mixed = COV && A.cur.coverage != 0u && t_mixed(G.pad);
            const float fx = floorf(xp), fy = floorf(yp);
            const float xr = floorf(xp + 0.5f), yr = floorf(yp + 0.5f); // within [-1, W] x [-1, H] by the range test above
            const bool snap = fabsf(xp - xr) <= HJR_TEMPORAL_SNAP && fabsf(yp - yr) <= HJR_TEMPORAL_SNAP;
            const int x0 = (int)(g_mixed ? xr : fx), y0 = (int)(g_mixed ? yr : fy);
            const float tx = xp - fx, ty = yp - fy;
            const int n_taps = g_mixed ? (snap ? 1 : 0) : 4;
            const float wk[4] = { g_mixed ? 1.0f : (1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty };
            const f3 view = gpos - V(A.cur.cam.pos[0], A.cur.cam.pos[1], A.cur.cam.pos[2]), ng = V(G.ng[0], G.ng[1], G.ng[2]);
            const float vv = t_dot(view, view), fh = A.cur.cam.f * H;
            const float fp2 = (vv * 4.0f) / (fh * fh), nn = t_dot(ng, ng), nv = t_dot(ng, view);
            const float lim_plane = ((HJR_TEMPORAL_K_PLANE * HJR_TEMPORAL_K_PLANE) * fp2) * nn;
            const float lim_dist = (((HJR_TEMPORAL_K_DIST * HJR_TEMPORAL_K_DIST) * fp2) * nn) * vv;
            const float* const m_cur = A.cur.m + (size_t)G.inst * 12u;
            float S = 0.0f, Cx = 0.0f, Cy = 0.0f, Cz = 0.0f, Vs = 0.0f, Hs = 0.0f;
            bool unknown = false;
            [[maybe_unused]] float M1 = 0.0f, M2 = 0.0f;
            constexpr int kUnroll = COV ? 4 : 1; // the loop shapes each instantiation was measured with: the coverage rules unrolled, the plain loop rolled
#pragma unroll kUnroll
            for (int k = 0; k < 4; k++) {
                if (k >= n_taps) continue;
                const int xt = x0 + (k & 1), yt = y0 + (k >> 1);
                if (xt < 0 || yt < 0 || xt >= (int)A.width || yt >= (int)A.height) continue;
                const size_t tap = (size_t)yt * A.width + (size_t)xt;
                const hjr_gbuffer_px T = A.prev.gbuf[tap];
                if (T.prim == 0xffffffffu || T.prim >= A.n_tris || T.inst != G.inst) continue; // (G.inst < n_instances: so is T.inst)
                if (COV && A.prev.coverage != 0u && (g_mixed ? T.pad != G.pad : t_mixed(T.pad))) continue; // rules 2' and 3'
                const f3 e = t_xf(A.prev.inv + (size_t)T.inst * 12u, V(T.pos[0], T.pos[1], T.pos[2])) - p_obj;
                const f3 D = t_lin(m_cur, e);
                const float nd = t_dot(ng, D);
                if (!(nd * nd <= lim_plane) || !(t_dot(D, D) * (nv * nv) <= lim_dist)) continue;
                const float4 pc = A.prev.color[tap];
                const float pv = A.prev.variance[tap];
                S = S + wk[k];
                Cx = Cx + pc.x * wk[k]; Cy = Cy + pc.y * wk[k]; Cz = Cz + pc.z * wk[k];
                unknown = unknown || !(pv < HJR_VARIANCE_UNKNOWN);
                Vs = Vs + fmaxf(pv, 0.0f) * wk[k];
                Hs = Hs + A.prev.history[tap] * wk[k];
                if constexpr (MOM) {
                    const float2 pm = A.prev.moments[tap];
                    M1 = M1 + pm.x * wk[k]; M2 = M2 + pm.y * wk[k];
                }
            }
            if (S > 0.0f) {
                TemporalPrev P;
                P.cx = Cx / S; P.cy = Cy / S; P.cz = Cz / S; P.v = Vs / S; P.h = Hs / S;
                P.unknown = unknown; P.inst = G.inst;
                if constexpr (MOM) { P.m1 = M1 / S; P.m2 = M2 / S; } else P.m1 = P.m2 = 0.0f;
                carried(P);
            }
        }
    }
}

// Step 4's blend (with the moments' part); RESP: as section RESPONSE has it, al and h answer to lambda first.
template <bool MOM, bool RESP>
__device__ __forceinline__ void hjr_temporal_blend(const TemporalPrev& P, float4 cc, float cv, [[maybe_unused]] float lum, [[maybe_unused]] float lambda, float4& out, float& var,
                                                   float& hist, [[maybe_unused]] float& m1, [[maybe_unused]] float& m2)
{
    hist = fminf(fmaxf(P.h + 1.0f, 1.0f), HJR_TEMPORAL_H_MAX);
    float al = fmaxf(1.0f / hist, HJR_TEMPORAL_ALPHA);
    if constexpr (RESP) {
        al = fmaxf(al, lambda);
        hist = lambda > 0.0f ? fminf(hist, 1.0f / al) : hist;
    }
    out.x = P.cx + (cc.x - P.cx) * al; out.y = P.cy + (cc.y - P.cy) * al; out.z = P.cz + (cc.z - P.cz) * al;
    const bool unknown = P.unknown || !(cv < HJR_VARIANCE_UNKNOWN);
    const float om = 1.0f - al;
    var = unknown ? HJR_VARIANCE_UNKNOWN : (om * om) * P.v + (al * al) * fmaxf(cv, 0.0f);
    if constexpr (MOM) {
        m1 = P.m1 + (lum - P.m1) * al; m2 = P.m2 + (lum * lum - P.m2) * al;
        if (hist >= HJR_TEMPORAL_MOMENTS_MIN) {
            const float kk = fmaxf(1.0f / hist, HJR_TEMPORAL_ALPHA / (2.0f - HJR_TEMPORAL_ALPHA));
            const float d = m2 - m1 * m1;
            const float mv = t_finite(d) ? fmaxf(d, 0.0f) * (kk / (1.0f - kk)) : HJR_VARIANCE_UNKNOWN;
            var = mv < HJR_VARIANCE_UNKNOWN ? mv : HJR_VARIANCE_UNKNOWN;
        }
    }
}

template <bool COV, bool MOM>
__global__ void __launch_bounds__(256) hjr_temporal_kernel(const TemporalArgs A)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= A.width || y >= A.height) return;
    const size_t pix = (size_t)y * A.width + x;
    const float4 cc = A.cur.color[pix];
    const float cv = A.cur.variance[pix];
    float4 out = cc;
    float var = cv, hist = 1.0f;
    [[maybe_unused]] float lum = 0.0f, m1 = 0.0f, m2 = 0.0f;
    if constexpr (MOM) { lum = (cc.x + cc.y) + cc.z; m1 = lum; m2 = lum * lum; }
    hjr_temporal_gather<COV, MOM>(A, pix, [&](const TemporalPrev& P) { hjr_temporal_blend<MOM, false>(P, cc, cv, lum, 0.0f, out, var, hist, m1, m2); });
    A.out.color[pix] = out;
    A.out.variance[pix] = var;
    A.out.history[pix] = hist;
    if constexpr (MOM) A.out.moments[pix] = make_float2(m1, m2);
}

// PRIOR (section PRIOR of the header comment): hjr_temporal_kernel's launch shape and gather, no colour of the current frame.  A.out and
// the current side's colour and variance are not looked at; the prior is an argument of its own, so TemporalArgs stays what it was.
template <bool COV>
__global__ void __launch_bounds__(256) hjr_temporal_prior_kernel(const TemporalArgs A, float4* __restrict__ prior)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= A.width || y >= A.height) return;
    const size_t pix = (size_t)y * A.width + x;
    float4 out = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
    hjr_temporal_gather<COV, false>(A, pix, [&](const TemporalPrev& P) {
        if (P.unknown) return;
        const float h = fminf(fmaxf(P.h + 1.0f, 1.0f), HJR_TEMPORAL_H_MAX);
        out = make_float4((P.cx + P.cy) + P.cz, P.v, fmaxf(1.0f / h, HJR_TEMPORAL_ALPHA), 0.0f);
    });
    prior[pix] = out;
}

// RESPONSE (section RESPONSE of the header comment).  A 256-thread workgroup owns a 16 x 16 pixel tile and stages the tile and a halo of
// HJR_TEMPORAL_RESP_R pixels in LDS: per cell lc, lc - lp and a member key (the instance of a carried pixel, RESP_NO_KEY for every other
// cell: restarted, outside the image), so that "q is a member of p's window" is one compare with G_p.inst.  Every thread gathers its own
// pixel (round 0, kept in registers for the blend) and the first RESP_HALO threads one halo cell each (round 1); after the one barrier every
// carried pixel takes its window sums from LDS in window order.  Three planes of RESP_ROWS rows with a row stride of RESP_STRIDE = 48
// floats: a wave's lanes are 4 rows of 16 pixels, ds_read_b32 conflicts within a 32-lane half (2 rows) over 32 banks, and 48 = 16 mod 32
// puts the second row's 16 banks beside the first's at every window offset (the row length 20 would be a 2-way conflict on 12 of 16 banks).
#define RESP_TILE 16
#define RESP_SIDE (RESP_TILE + 2 * HJR_TEMPORAL_RESP_R)                                  // 20 (22 with R = 3)
#define RESP_HALO (RESP_SIDE * RESP_SIDE - RESP_TILE * RESP_TILE)                        // 144 (228): at most one round of 256 threads
#define RESP_STRIDE 48
#define RESP_NO_KEY 0xffffffffu // (no carried pixel has it: G.inst < n_instances <= 0xffffffff)
static_assert(RESP_HALO <= 256 && RESP_SIDE <= RESP_STRIDE && RESP_STRIDE % 32 == 16, "one halo round, rows that fit, rows of a half on unlike banks");

template <bool COV, bool MOM>
__global__ void __launch_bounds__(256) hjr_temporal_resp_kernel(const TemporalArgs A)
{
    __shared__ float s_lc[RESP_SIDE * RESP_STRIDE], s_d[RESP_SIDE * RESP_STRIDE];
    __shared__ uint32_t s_key[RESP_SIDE * RESP_STRIDE];
    constexpr int R = HJR_TEMPORAL_RESP_R;
    const int tid = (int)threadIdx.x, lx = tid & (RESP_TILE - 1), ly = tid >> 4;
    // the thread's own pixel: what the blend needs stays in registers
    float4 own_cc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float own_cv = 0.0f, own_lc = 0.0f;
    bool own_carried = false, own_inside = false;
    TemporalPrev own;
    own.cx = own.cy = own.cz = own.v = own.h = own.m1 = own.m2 = 0.0f; own.unknown = false; own.inst = 0u;
#pragma unroll 1
    for (int round = 0; round < 2; round++) {
        int cx, cy; // the cell in the staged square
        if (round == 0) { cx = lx + R; cy = ly + R; }
        else {
            if (tid >= RESP_HALO) break;
            constexpr int kBand = R * RESP_SIDE; // cells of the rows above the tile, and of those below
            if (tid < 2 * kBand) { const int b = tid < kBand ? tid : tid - kBand; cy = b / RESP_SIDE + (tid < kBand ? 0 : RESP_TILE + R); cx = b % RESP_SIDE; }
            else { const int b = tid - 2 * kBand; cy = R + b / (2 * R); const int k = b % (2 * R); cx = k < R ? k : RESP_TILE + k; }
        }
        const int px = (int)(blockIdx.x * RESP_TILE) + cx - R, py = (int)(blockIdx.y * RESP_TILE) + cy - R;
        const bool inside = px >= 0 && py >= 0 && px < (int)A.width && py < (int)A.height;
        float lc = 0.0f, d = 0.0f;
        uint32_t key = RESP_NO_KEY;
        if (inside) {
            const size_t pix = (size_t)py * A.width + (size_t)px;
            const float4 cc = A.cur.color[pix];
            lc = (cc.x + cc.y) + cc.z;
            bool carried = false;
            hjr_temporal_gather<COV, MOM>(A, pix, [&](const TemporalPrev& P) {
                carried = true; d = lc - ((P.cx + P.cy) + P.cz); key = P.inst;
                if (round == 0) own = P;
            });
            if (round == 0) { own_cc = cc; own_cv = A.cur.variance[pix]; own_lc = lc; own_carried = carried; own_inside = true; }
        }
        const int cell = cy * RESP_STRIDE + cx;
        s_lc[cell] = lc; s_d[cell] = d; s_key[cell] = key;
    }
    __syncthreads();
    if (!own_inside) return;
    float4 out = own_cc;
    float var = own_cv, hist = 1.0f, lambda = 0.0f;
    [[maybe_unused]] float m1 = own_lc, m2 = own_lc * own_lc;
    if (own_carried) {
        float Sd = 0.0f, Sc = 0.0f, Sc2 = 0.0f;
        int n = 0;
#pragma unroll
        for (int dy = -R; dy <= R; dy++) {
#pragma unroll
            for (int dx = -R; dx <= R; dx++) {
                const int cell = (ly + R + dy) * RESP_STRIDE + (lx + R + dx);
                const bool member = s_key[cell] == own.inst;
                const float qc = s_lc[cell], qd = s_d[cell];
                n += member ? 1 : 0;
                Sd = member ? Sd + qd : Sd;
                Sc = member ? Sc + qc : Sc;
                Sc2 = member ? Sc2 + qc * qc : Sc2;
            }
        }
        const float nf = (float)n;
        const float mu_d = Sd / nf, mu_c = Sc / nf;
        const float var_c = fmaxf(Sc2 / nf - mu_c * mu_c, 0.0f);
        const float se = sqrtf(var_c / nf) + HJR_TEMPORAL_RESP_EPS;
        const float t = fabsf(mu_d) / se;
        lambda = n >= HJR_TEMPORAL_RESP_NMIN ? fminf(fmaxf((t - HJR_TEMPORAL_RESP_T0) / (HJR_TEMPORAL_RESP_T1 - HJR_TEMPORAL_RESP_T0), 0.0f), 1.0f) : 0.0f;
        hjr_temporal_blend<MOM, true>(own, own_cc, own_cv, own_lc, lambda, out, var, hist, m1, m2);
    }
    const size_t pix = (size_t)(blockIdx.y * RESP_TILE + ly) * A.width + (blockIdx.x * RESP_TILE + lx);
    A.out.color[pix] = out;
    A.out.variance[pix] = var;
    A.out.history[pix] = hist;
    if constexpr (MOM) A.out.moments[pix] = make_float2(m1, m2);
    A.out.response[pix] = lambda;
}
