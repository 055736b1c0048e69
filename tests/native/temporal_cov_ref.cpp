// CPU checker of the coverage G-buffer pass and of the coverage-aware accumulation (csrc/hjr_temporal.hip.h, sections COVERAGE G-BUFFER and
// COVERAGE-AWARE ACCUMULATION of its header comment), restated from that comment: fp32, every operation as written, built with
// -ffp-contract=off so that no multiply-add is fused (the triangle test's fused operations are explicit fmaf calls).
//   temporal_cov_ref gbuf W H SIDE N_ROWS N_TRIANGLES in.bin out.bin
//     in.bin: camera (pos, dir, up, right, f: 13 floats) | triangle rows [N_ROWS][12] floats (v0, v1, v2 world space, word 9 the prim id) |
//       tri_inst [N_TRIANGLES] u32 | material id [N_TRIANGLES] u32.   out.bin: [H][W] 48-byte records.   SIDE 0: the plain G-buffer (pad = 0).
//     Closest hits by brute force over all rows: smallest t, ties to the smaller prim id (DESIGN.md §4 rule 3).
//   temporal_cov_ref acc W H N_INSTANCES N_TRIANGLES HAVE_PREV PREV_COVERAGE CUR_COVERAGE in.bin out.bin [SNAP]
//     in.bin / out.bin as tests/native/temporal_ref.cpp's.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static const float UNKNOWN = 1e30f, ALPHA = 0.2f, K_PLANE = 1.0f, K_DIST = 3.0f;

struct Px { uint32_t prim, inst; float t, b1, b2; float pos[3]; float ng[3]; uint32_t pad; };
static_assert(sizeof(Px) == 48, "record size");
struct Vec { float x, y, z; };

static Vec mk(float x, float y, float z) { Vec v = { x, y, z }; return v; }
static Vec sub(Vec a, Vec b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static float dot(Vec a, Vec b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static Vec cross(Vec a, Vec b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static Vec xf(const float* M, Vec p)
{
    return mk(((M[0] * p.x + M[1] * p.y) + M[2] * p.z) + M[3], ((M[4] * p.x + M[5] * p.y) + M[6] * p.z) + M[7], ((M[8] * p.x + M[9] * p.y) + M[10] * p.z) + M[11]);
}
static Vec lin(const float* M, Vec d)
{
    return mk((M[0] * d.x + M[1] * d.y) + M[2] * d.z, (M[4] * d.x + M[5] * d.y) + M[6] * d.z, (M[8] * d.x + M[9] * d.y) + M[10] * d.z);
}
static bool finite_f(float x) { return std::fabs(x) <= FLT_MAX; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// ---------------------------------------------------------------------------------------------------------------- the coverage pass
// the canonical ray / triangle test: its multiply-adds are fused by name
static float dotf(Vec a, Vec b) { return std::fmaf(a.z, b.z, std::fmaf(a.y, b.y, a.x * b.x)); }
static Vec crossf(Vec a, Vec b) { return mk(std::fmaf(a.y, b.z, -(a.z * b.y)), std::fmaf(a.z, b.x, -(a.x * b.z)), std::fmaf(a.x, b.y, -(a.y * b.x))); }
static bool ray_tri(Vec v0, Vec v1, Vec v2, Vec o, Vec d, float tmin, float tmax, float& t, float& b1, float& b2)
{
    const Vec e1 = sub(v1, v0), e2 = sub(v2, v0), p = crossf(d, e2);
    const float det = dotf(e1, p), inv = 1.0f / det;
    const Vec tv = sub(o, v0);
    const float u = dotf(tv, p) * inv;
    const Vec q = crossf(tv, e1);
    const float v = dotf(d, q) * inv, tt = dotf(e2, q) * inv;
    if (!(det != 0.0f) || !(u >= 0.0f) || !(u <= 1.0f) || !(v >= 0.0f) || !(u + v <= 1.0f) || !(tt > tmin) || !(tt < tmax)) return false;
    t = tt; b1 = u; b2 = v;
    return true;
}

struct Found { bool hit; uint32_t prim, inst, mat; float t, b1, b2; Vec pos, ng; };

static Found first_hit(const float* cam, const std::vector<float>& rows, size_t n_rows, uint32_t n_tris, const std::vector<uint32_t>& tri_inst,
                       const std::vector<uint32_t>& tri_mat, float W, float H, float sx, float sy)
{
    const float u = (2.0f * sx - W) / H, v = (2.0f * sy - H) / H, f = cam[12];
    Vec d = mk((cam[3] * f + cam[9] * u) + cam[6] * v, (cam[4] * f + cam[10] * u) + cam[7] * v, (cam[5] * f + cam[11] * u) + cam[8] * v);
    const float inv_len = 1.0f / std::sqrt((d.x * d.x + d.y * d.y) + d.z * d.z);
    d = mk(d.x * inv_len, d.y * inv_len, d.z * inv_len);
    const Vec o = mk(cam[0], cam[1], cam[2]);
    Found best;
    memset(&best, 0, sizeof(best));
    best.prim = 0xffffffffu;
    size_t best_row = 0;
    for (size_t k = 0; k < n_rows; k++) {
        const float* g = &rows[k * 12];
        float t, b1, b2;
        if (!ray_tri(mk(g[0], g[1], g[2]), mk(g[3], g[4], g[5]), mk(g[6], g[7], g[8]), o, d, 0.001f, 1e16f, t, b1, b2)) continue;
        const uint32_t prim = bits(g[9]);
        if (best.prim == 0xffffffffu || t < best.t || (t == best.t && prim < best.prim)) { best.prim = prim; best.t = t; best.b1 = b1; best.b2 = b2; best_row = k; }
    }
    best.hit = best.prim != 0xffffffffu && best.prim < n_tris;
    if (best.hit) {
        const float* g = &rows[best_row * 12];
        const Vec v0 = mk(g[0], g[1], g[2]), v1 = mk(g[3], g[4], g[5]), v2 = mk(g[6], g[7], g[8]);
        const float w0 = (1.0f - best.b1) - best.b2;
        best.pos = mk((v0.x * w0 + v1.x * best.b1) + v2.x * best.b2, (v0.y * w0 + v1.y * best.b1) + v2.y * best.b2, (v0.z * w0 + v1.z * best.b1) + v2.z * best.b2);
        best.ng = cross(sub(v1, v0), sub(v2, v0));
        best.inst = tri_inst[best.prim];
        best.mat = tri_mat[best.prim];
    }
    return best;
}

static int run_gbuf(char** a)
{
    const int Wi = atoi(a[0]), Hi = atoi(a[1]), side = atoi(a[2]);
    const size_t n_rows = strtoul(a[3], nullptr, 10);
    const uint32_t n_tris = (uint32_t)strtoul(a[4], nullptr, 10);
    if (Wi <= 0 || Hi <= 0 || !(side == 0 || (side >= 2 && side <= 4))) { fprintf(stderr, "bad size or side\n"); return 2; }
    float cam[13];
    std::vector<float> rows(n_rows * 12);
    std::vector<uint32_t> tri_inst(n_tris), tri_mat(n_tris);
    FILE* f = fopen(a[5], "rb");
    if (!f) { perror("in"); return 1; }
    const bool ok = fread(cam, 4, 13, f) == 13 && fread(rows.data(), 4, rows.size(), f) == rows.size() && fread(tri_inst.data(), 4, n_tris, f) == n_tris &&
                    fread(tri_mat.data(), 4, n_tris, f) == n_tris;
    fclose(f);
    if (!ok) { fprintf(stderr, "short input\n"); return 1; }
    std::vector<Px> out((size_t)Wi * Hi);
    const float W = (float)Wi, H = (float)Hi;
    for (int py = 0; py < Hi; py++)
        for (int px = 0; px < Wi; px++) {
            Px& r = out[(size_t)py * Wi + px];
            memset(&r, 0, sizeof(r));
            r.prim = 0xffffffffu;
            const Found c = first_hit(cam, rows, n_rows, n_tris, tri_inst, tri_mat, W, H, (float)px + 0.5f, (float)py + 0.5f);
            float lim = 0.0f;
            if (c.hit) {
                r.prim = c.prim; r.inst = c.inst; r.t = c.t; r.b1 = c.b1; r.b2 = c.b2;
                r.pos[0] = c.pos.x; r.pos[1] = c.pos.y; r.pos[2] = c.pos.z;
                r.ng[0] = c.ng.x; r.ng[1] = c.ng.y; r.ng[2] = c.ng.z;
                const Vec view = sub(c.pos, mk(cam[0], cam[1], cam[2]));
                const float vv = dot(view, view), fh = cam[12] * H;
                const float fp2 = (vv * 4.0f) / (fh * fh), nn = dot(c.ng, c.ng);
                lim = ((K_PLANE * K_PLANE) * fp2) * nn;
            }
            if (side == 0) continue;
            uint32_t same = 0;
            for (int j = 0; j < side; j++)
                for (int i = 0; i < side; i++) {
                    const float ox = ((float)i + 0.5f) / (float)side, oy = ((float)j + 0.5f) / (float)side;
                    const Found s = first_hit(cam, rows, n_rows, n_tris, tri_inst, tri_mat, W, H, (float)px + ox, (float)py + oy);
                    if (!c.hit) { if (!s.hit) same++; continue; }
                    if (!s.hit || s.inst != c.inst || s.mat != c.mat) continue;
                    const float nd = dot(c.ng, sub(s.pos, c.pos));
                    if (nd * nd <= lim) same++;
                }
            r.pad = same | ((uint32_t)(side * side) << 8);
        }
    f = fopen(a[6], "wb");
    if (!f) { perror("out"); return 1; }
    fwrite(out.data(), sizeof(Px), out.size(), f);
    fclose(f);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the accumulation
struct Side {
    float cam[13]; // pos 0..2, dir 3..5, up 6..8, right 9..11, f 12
    std::vector<float> m, inv, color, variance, history;
    std::vector<Px> g;
};

static bool read_side(FILE* f, Side& s, size_t n_inst, size_t npx, bool with_history)
{
    s.m.resize(n_inst * 12); s.inv.resize(n_inst * 12); s.g.resize(npx); s.color.resize(npx * 4); s.variance.resize(npx);
    if (with_history) s.history.resize(npx);
    bool ok = fread(s.cam, 4, 13, f) == 13;
    ok = ok && fread(s.m.data(), 4, s.m.size(), f) == s.m.size() && fread(s.inv.data(), 4, s.inv.size(), f) == s.inv.size();
    ok = ok && fread(s.g.data(), sizeof(Px), npx, f) == npx && fread(s.color.data(), 4, npx * 4, f) == npx * 4 && fread(s.variance.data(), 4, npx, f) == npx;
    if (with_history) ok = ok && fread(s.history.data(), 4, npx, f) == npx;
    return ok;
}

static bool mixed(uint32_t pad)
{
    const uint32_t total = (pad >> 8) & 0xffu, same = pad & 0xffu;
    return total > 0u && same < total;
}

static int run_acc(int argc, char** a)
{
    const int Wi = atoi(a[0]), Hi = atoi(a[1]);
    const uint32_t n_inst = (uint32_t)strtoul(a[2], nullptr, 10), n_tris = (uint32_t)strtoul(a[3], nullptr, 10);
    const bool have_prev = atoi(a[4]) != 0;
    const bool prev_cov = have_prev && strtoul(a[5], nullptr, 10) != 0, cur_cov = strtoul(a[6], nullptr, 10) != 0;
    const float snap_lim = argc > 9 ? (float)atof(a[9]) : 0.125f;
    if (Wi <= 0 || Hi <= 0) { fprintf(stderr, "bad size\n"); return 2; }
    const size_t npx = (size_t)Wi * Hi;
    Side prev, cur;
    FILE* f = fopen(a[7], "rb");
    if (!f) { perror("in"); return 1; }
    const bool ok = (!have_prev || read_side(f, prev, n_inst, npx, true)) && read_side(f, cur, n_inst, npx, false);
    fclose(f);
    if (!ok) { fprintf(stderr, "short input\n"); return 1; }
    std::vector<float> oc(npx * 4), ov(npx), oh(npx);
    const float W = (float)Wi, H = (float)Hi;
    for (int y = 0; y < Hi; y++)
        for (int x = 0; x < Wi; x++) {
            const size_t pix = (size_t)y * Wi + x;
            for (int k = 0; k < 4; k++) oc[pix * 4 + k] = cur.color[pix * 4 + k]; // RESTART values
            ov[pix] = cur.variance[pix];
            oh[pix] = 1.0f;
            const Px& G = cur.g[pix];
            // 1.
            if (!have_prev || G.prim == 0xffffffffu || G.prim >= n_tris || G.inst >= n_inst) continue;
            // 2.
            const Vec gpos = mk(G.pos[0], G.pos[1], G.pos[2]);
            const Vec p_obj = xf(&cur.inv[(size_t)G.inst * 12], gpos);
            const Vec p_prev = xf(&prev.m[(size_t)G.inst * 12], p_obj);
            const Vec w = sub(p_prev, mk(prev.cam[0], prev.cam[1], prev.cam[2]));
            const float pf = prev.cam[12];
            const Vec a3 = mk(prev.cam[3] * pf, prev.cam[4] * pf, prev.cam[5] * pf), c3 = mk(prev.cam[6], prev.cam[7], prev.cam[8]), b3 = mk(prev.cam[9], prev.cam[10], prev.cam[11]);
            const Vec bc = cross(b3, c3);
            const float det = dot(a3, bc);
            const float s = dot(w, bc) / det, su = dot(a3, cross(w, c3)) / det, sv = dot(a3, cross(b3, w)) / det;
            const float u = su / s, v = sv / s;
            if (!(det != 0.0f) || !(s > 0.0f) || !finite_f(s) || !finite_f(u) || !finite_f(v)) continue;
            const float xp = (u * H + W) * 0.5f - 0.5f, yp = (v * H + H) * 0.5f - 0.5f;
            if (!(xp >= -1.0f) || !(xp < W) || !(yp >= -1.0f) || !(yp < H)) continue;
            // the taps: rule 3's four, or rule 2''s one
            int tap_x[4], tap_y[4], n_taps = 4;
            float wk[4];
            const bool g_mixed = cur_cov && mixed(G.pad);
            if (g_mixed) {
                const float xr = std::floor(xp + 0.5f), yr = std::floor(yp + 0.5f);
                if (!(std::fabs(xp - xr) <= snap_lim) || !(std::fabs(yp - yr) <= snap_lim)) continue;
                n_taps = 1; tap_x[0] = (int)xr; tap_y[0] = (int)yr; wk[0] = 1.0f;
            } else {
                const float fx = std::floor(xp), fy = std::floor(yp);
                const int x0 = (int)fx, y0 = (int)fy;
                const float tx = xp - fx, ty = yp - fy;
                wk[0] = (1.0f - tx) * (1.0f - ty); wk[1] = tx * (1.0f - ty); wk[2] = (1.0f - tx) * ty; wk[3] = tx * ty;
                for (int k = 0; k < 4; k++) { tap_x[k] = x0 + (k & 1); tap_y[k] = y0 + (k >> 1); }
            }
            // 3.
            const Vec view = sub(gpos, mk(cur.cam[0], cur.cam[1], cur.cam[2])), ng = mk(G.ng[0], G.ng[1], G.ng[2]);
            const float vv = dot(view, view), fh = cur.cam[12] * H;
            const float fp2 = (vv * 4.0f) / (fh * fh), nn = dot(ng, ng), nv = dot(ng, view);
            const float lim_plane = ((K_PLANE * K_PLANE) * fp2) * nn, lim_dist = (((K_DIST * K_DIST) * fp2) * nn) * vv;
            float S = 0.0f, C[3] = { 0.0f, 0.0f, 0.0f }, Vs = 0.0f, Hs = 0.0f;
            bool unknown = false;
            for (int k = 0; k < n_taps; k++) {
                const int xt = tap_x[k], yt = tap_y[k];
                if (xt < 0 || yt < 0 || xt >= Wi || yt >= Hi) continue;
                const size_t tap = (size_t)yt * Wi + xt;
                const Px& T = prev.g[tap];
                if (T.prim == 0xffffffffu || T.prim >= n_tris || T.inst != G.inst) continue;
                if (g_mixed) { if (prev_cov && T.pad != G.pad) continue; } // 2'
                else if (prev_cov && mixed(T.pad)) continue;              // 3'
                const Vec e = sub(xf(&prev.inv[(size_t)T.inst * 12], mk(T.pos[0], T.pos[1], T.pos[2])), p_obj);
                const Vec D = lin(&cur.m[(size_t)G.inst * 12], e);
                const float nd = dot(ng, D);
                if (!(nd * nd <= lim_plane)) continue;
                if (!(dot(D, D) * (nv * nv) <= lim_dist)) continue;
                // 4.
                const float pv = prev.variance[tap];
                S = S + wk[k];
                for (int q = 0; q < 3; q++) C[q] = C[q] + prev.color[tap * 4 + q] * wk[k];
                if (!(pv < UNKNOWN)) unknown = true;
                Vs = Vs + (pv > 0.0f ? pv : 0.0f) * wk[k]; // fmaxf(pv, 0): NaN -> 0
                Hs = Hs + prev.history[tap] * wk[k];
            }
            if (!(S > 0.0f)) continue;
            const float v_prev = Vs / S, h_prev = Hs / S;
            float h = h_prev + 1.0f;
            h = h > 1.0f ? h : 1.0f;   // fmaxf(., 1): NaN -> 1
            h = h < 64.0f ? h : 64.0f; // fminf(., 64)
            const float r = 1.0f / h, al = r > ALPHA ? r : ALPHA;
            for (int q = 0; q < 3; q++) {
                const float cp = C[q] / S;
                oc[pix * 4 + q] = cp + (cur.color[pix * 4 + q] - cp) * al;
            }
            const float cv = cur.variance[pix];
            if (!(cv < UNKNOWN)) unknown = true;
            const float om = 1.0f - al;
            ov[pix] = unknown ? UNKNOWN : (om * om) * v_prev + (al * al) * (cv > 0.0f ? cv : 0.0f);
            oh[pix] = h;
        }
    f = fopen(a[8], "wb");
    if (!f) { perror("out"); return 1; }
    fwrite(oc.data(), 4, oc.size(), f); fwrite(ov.data(), 4, ov.size(), f); fwrite(oh.data(), 4, oh.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 9 && strcmp(argv[1], "gbuf") == 0) return run_gbuf(argv + 2);
    if ((argc == 11 || argc == 12) && strcmp(argv[1], "acc") == 0) return run_acc(argc - 2, argv + 2);
    fprintf(stderr, "usage: temporal_cov_ref gbuf W H SIDE N_ROWS N_TRIANGLES in out\n"
                    "       temporal_cov_ref acc W H N_INSTANCES N_TRIANGLES HAVE_PREV PREV_COVERAGE CUR_COVERAGE in out [SNAP]\n");
    return 2;
}
