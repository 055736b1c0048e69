// CPU checker of the temporal accumulation rule (csrc/hjr_temporal.hip.h, section ACCUMULATION of its header comment), restated from that
// comment: fp32, every operation as written, built with -ffp-contract=off so that no multiply-add is fused.
//   temporal_ref W H N_INSTANCES N_TRIANGLES HAVE_PREV in.bin out.bin [K_PLANE K_DIST]
// in.bin: per side (the previous frame first, if HAVE_PREV; then the current one):  camera (pos, dir, up, right, f: 13 floats) |
//   transforms [n][12] | inverse transforms [n][12] | G-buffer [H][W] 48-byte records | colour [H][W][4] | variance [H][W] | (previous
//   side only) history [H][W].   out.bin: colour [H][W][4] | variance [H][W] | history [H][W].
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static const float UNKNOWN = 1e30f, ALPHA = 0.2f;

struct Px { uint32_t prim, inst; float t, b1, b2; float pos[3]; float ng[3]; uint32_t pad; };
static_assert(sizeof(Px) == 48, "record size");
struct Vec { float x, y, z; };
struct Side {
    float cam[13]; // pos 0..2, dir 3..5, up 6..8, right 9..11, f 12
    std::vector<float> m, inv, color, variance, history;
    std::vector<Px> g;
};

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

int main(int argc, char** argv)
{
    if (argc != 8 && argc != 10) { fprintf(stderr, "usage: temporal_ref W H N_INSTANCES N_TRIANGLES HAVE_PREV in out [K_PLANE K_DIST]\n"); return 2; }
    const int Wi = atoi(argv[1]), Hi = atoi(argv[2]);
    const uint32_t n_inst = (uint32_t)strtoul(argv[3], nullptr, 10), n_tris = (uint32_t)strtoul(argv[4], nullptr, 10);
    const bool have_prev = atoi(argv[5]) != 0;
    const float k_plane = argc == 10 ? (float)atof(argv[8]) : 1.0f, k_dist = argc == 10 ? (float)atof(argv[9]) : 3.0f;
    const size_t npx = (size_t)Wi * Hi;
    Side prev, cur;
    FILE* f = fopen(argv[6], "rb");
    if (!f) { perror("in"); return 1; }
    if ((have_prev && !read_side(f, prev, n_inst, npx, true)) || !read_side(f, cur, n_inst, npx, false)) { fprintf(stderr, "short input\n"); return 1; }
    fclose(f);
    std::vector<float> oc(npx * 4), ov(npx), oh(npx);
    const float W = (float)Wi, H = (float)Hi;
    for (int y = 0; y < Hi; y++)
        for (int x = 0; x < Wi; x++) {
            const size_t pix = (size_t)y * Wi + x;
            // RESTART values
            for (int k = 0; k < 4; k++) oc[pix * 4 + k] = cur.color[pix * 4 + k];
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
            const Vec a = mk(prev.cam[3] * pf, prev.cam[4] * pf, prev.cam[5] * pf), c = mk(prev.cam[6], prev.cam[7], prev.cam[8]), b = mk(prev.cam[9], prev.cam[10], prev.cam[11]);
            const Vec bc = cross(b, c);
            const float det = dot(a, bc);
            const float s = dot(w, bc) / det, su = dot(a, cross(w, c)) / det, sv = dot(a, cross(b, w)) / det;
            const float u = su / s, v = sv / s;
            if (!(det != 0.0f) || !(s > 0.0f) || !finite_f(s) || !finite_f(u) || !finite_f(v)) continue;
            const float xp = (u * H + W) * 0.5f - 0.5f, yp = (v * H + H) * 0.5f - 0.5f;
            if (!(xp >= -1.0f) || !(xp < W) || !(yp >= -1.0f) || !(yp < H)) continue;
            const float fx = std::floor(xp), fy = std::floor(yp);
            const int x0 = (int)fx, y0 = (int)fy;
            const float tx = xp - fx, ty = yp - fy;
            // 3.
            const float wk[4] = { (1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty };
            const Vec view = sub(gpos, mk(cur.cam[0], cur.cam[1], cur.cam[2])), ng = mk(G.ng[0], G.ng[1], G.ng[2]);
            const float vv = dot(view, view), fh = cur.cam[12] * H;
            const float fp2 = (vv * 4.0f) / (fh * fh), nn = dot(ng, ng), nv = dot(ng, view);
            const float lim_plane = ((k_plane * k_plane) * fp2) * nn, lim_dist = (((k_dist * k_dist) * fp2) * nn) * vv;
            float S = 0.0f, C[3] = { 0.0f, 0.0f, 0.0f }, Vs = 0.0f, Hs = 0.0f;
            bool unknown = false;
            for (int k = 0; k < 4; k++) {
                const int xt = x0 + (k & 1), yt = y0 + (k >> 1);
                if (xt < 0 || yt < 0 || xt >= Wi || yt >= Hi) continue;
                const size_t tap = (size_t)yt * Wi + xt;
                const Px& T = prev.g[tap];
                if (T.prim == 0xffffffffu || T.prim >= n_tris || T.inst != G.inst) continue;
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
    f = fopen(argv[7], "wb");
    if (!f) { perror("out"); return 1; }
    fwrite(oc.data(), 4, oc.size(), f); fwrite(ov.data(), 4, ov.size(), f); fwrite(oh.data(), 4, oh.size(), f);
    fclose(f);
    return 0;
}
