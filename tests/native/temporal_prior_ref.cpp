// CPU checker of the prior of adaptive sampling's rule 11 (csrc/hjr_temporal.hip.h, section PRIOR of its header comment; the reprojection,
// the taps and their validity tests are sections ACCUMULATION and COVERAGE-AWARE ACCUMULATION of the same comment), restated from that
// comment: fp32, every operation as written, built with -ffp-contract=off so that no multiply-add is fused.  Includes nothing of csrc/.
//   temporal_prior_ref W H N_INSTANCES N_TRIANGLES HAVE_PREV PREV_COVERAGE CUR_COVERAGE in.bin out.bin
//     in.bin: [previous side, if HAVE_PREV: camera (pos, dir, up, right, f: 13 floats) | M [N_INSTANCES][12] | M^-1 [N_INSTANCES][12] |
//       G-buffer [H][W] 48-byte records | colour [H][W][4] | variance [H][W] | history [H][W]] | current side: camera | M | M^-1 | G-buffer
//       (the frame that is about to be rendered has no colour yet).
//     out.bin: the prior [H][W][4] floats: (lp, vp, al, 0).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static const float UNKNOWN = 1e30f, ALPHA = 0.2f, K_PLANE = 1.0f, K_DIST = 3.0f, SNAP = 0.125f, H_MAX = 64.0f;

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

struct Side {
    float cam[13]; // pos 0..2, dir 3..5, up 6..8, right 9..11, f 12
    std::vector<float> m, inv, color, variance, history;
    std::vector<Px> g;
};

// `images`: the previous side, which carries colour, variance and history behind its G-buffer
static bool read_side(FILE* f, Side& s, size_t n_inst, size_t npx, bool images)
{
    s.m.resize(n_inst * 12); s.inv.resize(n_inst * 12); s.g.resize(npx);
    bool ok = fread(s.cam, 4, 13, f) == 13;
    ok = ok && fread(s.m.data(), 4, s.m.size(), f) == s.m.size() && fread(s.inv.data(), 4, s.inv.size(), f) == s.inv.size();
    ok = ok && fread(s.g.data(), sizeof(Px), npx, f) == npx;
    if (!images) return ok;
    s.color.resize(npx * 4); s.variance.resize(npx); s.history.resize(npx);
    return ok && fread(s.color.data(), 4, npx * 4, f) == npx * 4 && fread(s.variance.data(), 4, npx, f) == npx && fread(s.history.data(), 4, npx, f) == npx;
}

static bool mixed(uint32_t pad)
{
    const uint32_t total = (pad >> 8) & 0xffu, same = pad & 0xffu;
    return total > 0u && same < total;
}

int main(int argc, char** argv)
{
    if (argc != 10) {
        fprintf(stderr, "usage: temporal_prior_ref W H N_INSTANCES N_TRIANGLES HAVE_PREV PREV_COVERAGE CUR_COVERAGE in out\n");
        return 2;
    }
    char** a = argv + 1;
    const int Wi = atoi(a[0]), Hi = atoi(a[1]);
    const uint32_t n_inst = (uint32_t)strtoul(a[2], nullptr, 10), n_tris = (uint32_t)strtoul(a[3], nullptr, 10);
    const bool have_prev = atoi(a[4]) != 0;
    const bool prev_cov = have_prev && strtoul(a[5], nullptr, 10) != 0, cur_cov = strtoul(a[6], nullptr, 10) != 0;
    if (Wi <= 0 || Hi <= 0) { fprintf(stderr, "bad size\n"); return 2; }
    const size_t npx = (size_t)Wi * Hi;
    Side prev, cur;
    FILE* f = fopen(a[7], "rb");
    if (!f) { perror("in"); return 1; }
    const bool ok = (!have_prev || read_side(f, prev, n_inst, npx, true)) && read_side(f, cur, n_inst, npx, false);
    fclose(f);
    if (!ok) { fprintf(stderr, "short input\n"); return 1; }
    std::vector<float> out(npx * 4);
    const float W = (float)Wi, H = (float)Hi;
    for (int y = 0; y < Hi; y++)
        for (int x = 0; x < Wi; x++) {
            const size_t pix = (size_t)y * Wi + x;
            float* const o = &out[pix * 4];
            o[0] = 0.0f; o[1] = 0.0f; o[2] = 1.0f; o[3] = 0.0f; // what every pixel without a usable history writes
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
                if (!(std::fabs(xp - xr) <= SNAP) || !(std::fabs(yp - yr) <= SNAP)) continue;
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
                // 4. up to the divides
                const float pv = prev.variance[tap];
                S = S + wk[k];
                for (int q = 0; q < 3; q++) C[q] = C[q] + prev.color[tap * 4 + q] * wk[k];
                if (!(pv < UNKNOWN)) unknown = true;
                Vs = Vs + (pv > 0.0f ? pv : 0.0f) * wk[k]; // fmaxf(pv, 0): NaN -> 0
                Hs = Hs + prev.history[tap] * wk[k];
            }
            if (!(S > 0.0f)) continue;
            // PRIOR
            if (unknown) continue;
            const float cr = C[0] / S, cg = C[1] / S, cb = C[2] / S, v_prev = Vs / S, h_prev = Hs / S;
            float h = h_prev + 1.0f;
            h = h > 1.0f ? h : 1.0f;     // fmaxf(., 1): NaN -> 1
            h = h < H_MAX ? h : H_MAX;   // fminf(., 64)
            const float r = 1.0f / h;
            o[0] = (cr + cg) + cb; o[1] = v_prev; o[2] = r > ALPHA ? r : ALPHA; o[3] = 0.0f;
        }
    f = fopen(a[8], "wb");
    if (!f) { perror("out"); return 1; }
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}
