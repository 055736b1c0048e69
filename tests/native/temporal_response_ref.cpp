// CPU checker of the temporal accumulation with the windowed change test (csrc/hjr_temporal.hip.h, sections ACCUMULATION, COVERAGE-AWARE
// ACCUMULATION, TEMPORAL MOMENTS and RESPONSE of its header comment), restated from that comment as a whole and not derived from the kernel
// or from the other checkers: fp32, every operation as written, built with -ffp-contract=off so that no multiply-add is fused.  Two passes
// over the image: the first reprojects every pixel and keeps what it gathered, the second takes the window sums and blends.
//   temporal_response_ref W H N_INSTANCES N_TRIANGLES HAVE_PREV PREV_COVERAGE CUR_COVERAGE MOMENTS RESPONSE in.bin out.bin [R]
// in.bin: per side (the previous frame first, if HAVE_PREV; then the current one):  camera (pos, dir, up, right, f: 13 floats) |
//   transforms [n][12] | inverse transforms [n][12] | G-buffer [H][W] 48-byte records | colour [H][W][4] | variance [H][W] | (previous side
//   only) history [H][W] | (previous side only, if MOMENTS) moments [H][W][2].
// out.bin: colour [H][W][4] | variance [H][W] | history [H][W] | (if MOMENTS) moments [H][W][2] | (if RESPONSE) lambda [H][W].
// RESPONSE 0 is the rule without the change test (tests/native/temporal_moments_ref.cpp's).  R overrides the window radius (default 2).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

const float UNKNOWN_VAR = 1e30f, ALPHA = 0.2f, SNAP = 0.125f, PLANE_K = 1.0f, DIST_K = 3.0f, LEN_MAX = 64.0f, MOMENTS_FROM = 4.0f;
const float RESP_T0 = 3.0f, RESP_T1 = 6.0f, RESP_EPS = 1e-3f;
const int RESP_NMIN = 5;
const uint32_t MISS = 0xffffffffu;

struct Rec { uint32_t prim, inst; float t, b1, b2, pos[3], ng[3]; uint32_t pad; };
static_assert(sizeof(Rec) == 48, "record size");
struct Cam { float pos[3], dir[3], up[3], right[3], f; };
static_assert(sizeof(Cam) == 52, "camera size");
struct Vec { float x, y, z; };

struct Side {
    Cam cam;
    std::vector<float> m, minv, rgba, var, len, mom;
    std::vector<Rec> rec;
};

bool read_floats(FILE* f, std::vector<float>& v, size_t n) { v.resize(n); return fread(v.data(), 4, n, f) == n; }
bool read_side(FILE* f, Side& s, size_t n_inst, size_t n_px, bool prev, bool moments)
{
    if (fread(&s.cam, sizeof(Cam), 1, f) != 1) return false;
    if (!read_floats(f, s.m, n_inst * 12) || !read_floats(f, s.minv, n_inst * 12)) return false;
    s.rec.resize(n_px);
    if (fread(s.rec.data(), sizeof(Rec), n_px, f) != n_px) return false;
    if (!read_floats(f, s.rgba, n_px * 4) || !read_floats(f, s.var, n_px)) return false;
    if (prev && !read_floats(f, s.len, n_px)) return false;
    return !(prev && moments) || read_floats(f, s.mom, n_px * 2);
}

Vec vec(const float* p) { return Vec{ p[0], p[1], p[2] }; }
Vec sub(Vec a, Vec b) { return Vec{ a.x - b.x, a.y - b.y, a.z - b.z }; }
float dot(Vec a, Vec b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
Vec cross(Vec a, Vec b) { return Vec{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
Vec point(const float* m, Vec p)
{
    float o[3];
    for (int i = 0; i < 3; i++) o[i] = ((m[4 * i] * p.x + m[4 * i + 1] * p.y) + m[4 * i + 2] * p.z) + m[4 * i + 3];
    return vec(o);
}
Vec direction(const float* m, Vec d)
{
    float o[3];
    for (int i = 0; i < 3; i++) o[i] = (m[4 * i] * d.x + m[4 * i + 1] * d.y) + m[4 * i + 2] * d.z;
    return vec(o);
}
bool finite_f(float x) { return std::fabs(x) <= FLT_MAX; }
float fmax_c(float a, float b) { return a > b ? a : b; } // fmaxf(a, b) with b no NaN: a NaN a gives b
float fmin_c(float a, float b) { return a < b ? a : b; } // fminf(a, b) with b no NaN
bool mixed(uint32_t pad) { const uint32_t total = (pad >> 8) & 0xffu; return total > 0u && (pad & 0xffu) < total; }
float lum3(const float* c) { return (c[0] + c[1]) + c[2]; }

struct Gathered { bool carried = false, unknown = false; float c[3] = { 0, 0, 0 }, v = 0, h = 0, m1 = 0, m2 = 0; };

struct Task {
    int w = 0, h = 0, radius = 2;
    uint32_t n_inst = 0, n_tris = 0;
    bool have_prev = false, prev_cov = false, cur_cov = false, moments = false, response = false;
    Side prev, cur;

    bool hit(const Rec& r) const { return r.prim != MISS && r.prim < n_tris; }

    // steps 1 to 4 up to c_prev, v_prev, h_prev (and m1p, m2p)
    Gathered gather(size_t pix) const
    {
        Gathered g;
        const Rec& G = cur.rec[pix];
        if (!have_prev || !hit(G) || G.inst >= n_inst) return g;
        const float W = (float)w, H = (float)h;
        const Vec gp = vec(G.pos), po = point(&cur.minv[(size_t)G.inst * 12], gp), pp = point(&prev.m[(size_t)G.inst * 12], po);
        const Vec wv = sub(pp, vec(prev.cam.pos));
        const Vec a = Vec{ prev.cam.dir[0] * prev.cam.f, prev.cam.dir[1] * prev.cam.f, prev.cam.dir[2] * prev.cam.f }, b = vec(prev.cam.right), c = vec(prev.cam.up);
        const Vec bc = cross(b, c);
        const float det = dot(a, bc);
        const float s = dot(wv, bc) / det, su = dot(a, cross(wv, c)) / det, sv = dot(a, cross(b, wv)) / det;
        const float u = su / s, v = sv / s;
        if (!(det != 0.0f) || !(s > 0.0f) || !finite_f(s) || !finite_f(u) || !finite_f(v)) return g;
        const float xp = (u * H + W) * 0.5f - 0.5f, yp = (v * H + H) * 0.5f - 0.5f;
        if (!(xp >= -1.0f) || !(xp < W) || !(yp >= -1.0f) || !(yp < H)) return g;
        struct Tap { int x, y; float wt; } taps[4];
        int n_taps = 0;
        const bool g_mixed = cur_cov && mixed(G.pad);
        if (g_mixed) {
            const float xr = std::floor(xp + 0.5f), yr = std::floor(yp + 0.5f);
            if (!(std::fabs(xp - xr) <= SNAP) || !(std::fabs(yp - yr) <= SNAP)) return g;
            taps[n_taps++] = Tap{ (int)xr, (int)yr, 1.0f };
        } else {
            const float fx = std::floor(xp), fy = std::floor(yp), tx = xp - fx, ty = yp - fy;
            const int x0 = (int)fx, y0 = (int)fy;
            taps[n_taps++] = Tap{ x0, y0, (1.0f - tx) * (1.0f - ty) };
            taps[n_taps++] = Tap{ x0 + 1, y0, tx * (1.0f - ty) };
            taps[n_taps++] = Tap{ x0, y0 + 1, (1.0f - tx) * ty };
            taps[n_taps++] = Tap{ x0 + 1, y0 + 1, tx * ty };
        }
        const Vec view = sub(gp, vec(cur.cam.pos)), ng = vec(G.ng);
        const float vv = dot(view, view), fh = cur.cam.f * H, fp2 = (vv * 4.0f) / (fh * fh), nn = dot(ng, ng), nv = dot(ng, view);
        const float plane_lim = ((PLANE_K * PLANE_K) * fp2) * nn, dist_lim = (((DIST_K * DIST_K) * fp2) * nn) * vv;
        float S = 0.0f, C[3] = { 0.0f, 0.0f, 0.0f }, V = 0.0f, L = 0.0f, M1 = 0.0f, M2 = 0.0f;
        for (int k = 0; k < n_taps; k++) {
            const Tap& t = taps[k];
            if (t.x < 0 || t.y < 0 || t.x >= w || t.y >= h) continue;
            const size_t q = (size_t)t.y * w + t.x;
            const Rec& T = prev.rec[q];
            if (!hit(T) || T.inst != G.inst) continue;
            if (prev_cov && (g_mixed ? T.pad != G.pad : mixed(T.pad))) continue;
            const Vec e = sub(point(&prev.minv[(size_t)T.inst * 12], vec(T.pos)), po);
            const Vec D = direction(&cur.m[(size_t)G.inst * 12], e);
            const float nd = dot(ng, D);
            if (!(nd * nd <= plane_lim) || !(dot(D, D) * (nv * nv) <= dist_lim)) continue;
            S = S + t.wt;
            for (int ch = 0; ch < 3; ch++) C[ch] = C[ch] + prev.rgba[q * 4 + ch] * t.wt;
            const float pv = prev.var[q];
            if (!(pv < UNKNOWN_VAR)) g.unknown = true;
            V = V + fmax_c(pv, 0.0f) * t.wt;
            L = L + prev.len[q] * t.wt;
            if (moments) { M1 = M1 + prev.mom[q * 2] * t.wt; M2 = M2 + prev.mom[q * 2 + 1] * t.wt; }
        }
        if (!(S > 0.0f)) return g;
        g.carried = true;
        for (int ch = 0; ch < 3; ch++) g.c[ch] = C[ch] / S;
        g.v = V / S; g.h = L / S;
        if (moments) { g.m1 = M1 / S; g.m2 = M2 / S; }
        return g;
    }

    // section RESPONSE: lambda of the carried pixel (x, y)
    float lambda(const std::vector<Gathered>& all, int x, int y) const
    {
        const uint32_t inst = cur.rec[(size_t)y * w + x].inst;
        float Sd = 0.0f, Sc = 0.0f, Sc2 = 0.0f;
        int n = 0;
        for (int dy = -radius; dy <= radius; dy++)
            for (int dx = -radius; dx <= radius; dx++) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
                const size_t q = (size_t)qy * w + qx;
                if (!hit(cur.rec[q]) || cur.rec[q].inst != inst || !all[q].carried) continue;
                const float lc = lum3(&cur.rgba[q * 4]), lp = lum3(all[q].c);
                Sd = Sd + (lc - lp);
                Sc = Sc + lc;
                Sc2 = Sc2 + lc * lc;
                n++;
            }
        const float nf = (float)n;
        const float mu_d = Sd / nf, mu_c = Sc / nf;
        const float var_c = fmax_c(Sc2 / nf - mu_c * mu_c, 0.0f);
        const float se = std::sqrt(var_c / nf) + RESP_EPS;
        const float t = std::fabs(mu_d) / se;
        if (n < RESP_NMIN) return 0.0f;
        return fmin_c(fmax_c((t - RESP_T0) / (RESP_T1 - RESP_T0), 0.0f), 1.0f);
    }
};

} // namespace

int main(int argc, char** argv)
{
    if (argc != 12 && argc != 13) {
        fprintf(stderr, "usage: temporal_response_ref W H N_INSTANCES N_TRIANGLES HAVE_PREV PREV_COVERAGE CUR_COVERAGE MOMENTS RESPONSE in out [R]\n");
        return 2;
    }
    Task t;
    t.w = atoi(argv[1]); t.h = atoi(argv[2]);
    t.n_inst = (uint32_t)strtoul(argv[3], nullptr, 10); t.n_tris = (uint32_t)strtoul(argv[4], nullptr, 10);
    t.have_prev = atoi(argv[5]) != 0;
    t.prev_cov = t.have_prev && strtoul(argv[6], nullptr, 10) != 0; t.cur_cov = strtoul(argv[7], nullptr, 10) != 0;
    t.moments = atoi(argv[8]) != 0; t.response = atoi(argv[9]) != 0;
    if (argc == 13) t.radius = atoi(argv[12]);
    if (t.w <= 0 || t.h <= 0 || t.radius < 0 || t.radius > 8) { fprintf(stderr, "bad size\n"); return 2; }
    const size_t n_px = (size_t)t.w * t.h;
    FILE* f = fopen(argv[10], "rb");
    if (!f) { perror("in"); return 1; }
    const bool ok = (!t.have_prev || read_side(f, t.prev, t.n_inst, n_px, true, t.moments)) && read_side(f, t.cur, t.n_inst, n_px, false, false);
    fclose(f);
    if (!ok) { fprintf(stderr, "short input\n"); return 1; }

    std::vector<Gathered> all(n_px);
    for (size_t pix = 0; pix < n_px; pix++) all[pix] = t.gather(pix);

    std::vector<float> o_rgba(n_px * 4), o_var(n_px), o_len(n_px), o_mom(t.moments ? n_px * 2 : 0), o_lam(t.response ? n_px : 0);
    for (int y = 0; y < t.h; y++)
        for (int x = 0; x < t.w; x++) {
            const size_t pix = (size_t)y * t.w + x;
            const Gathered& g = all[pix];
            const float* cc = &t.cur.rgba[pix * 4];
            const float cv = t.cur.var[pix], l = lum3(cc);
            float rgba[4] = { cc[0], cc[1], cc[2], cc[3] }, var = cv, len = 1.0f, m1 = l, m2 = l * l, lam = 0.0f;
            if (g.carried) {
                len = fmin_c(fmax_c(g.h + 1.0f, 1.0f), LEN_MAX);
                float al = fmax_c(1.0f / len, ALPHA);
                if (t.response) {
                    lam = t.lambda(all, x, y);
                    al = fmax_c(al, lam);
                    if (lam > 0.0f) len = fmin_c(len, 1.0f / al);
                }
                for (int ch = 0; ch < 3; ch++) rgba[ch] = g.c[ch] + (cc[ch] - g.c[ch]) * al;
                const bool unknown = g.unknown || !(cv < UNKNOWN_VAR);
                const float om = 1.0f - al;
                var = unknown ? UNKNOWN_VAR : (om * om) * g.v + (al * al) * fmax_c(cv, 0.0f);
                if (t.moments) {
                    m1 = g.m1 + (l - g.m1) * al;
                    m2 = g.m2 + (l * l - g.m2) * al;
                    if (len >= MOMENTS_FROM) {
                        const float k = fmax_c(1.0f / len, ALPHA / (2.0f - ALPHA));
                        const float d = m2 - m1 * m1;
                        const float mv = finite_f(d) ? fmax_c(d, 0.0f) * (k / (1.0f - k)) : UNKNOWN_VAR;
                        var = mv < UNKNOWN_VAR ? mv : UNKNOWN_VAR;
                    }
                }
            }
            for (int ch = 0; ch < 4; ch++) o_rgba[pix * 4 + ch] = rgba[ch];
            o_var[pix] = var; o_len[pix] = len;
            if (t.moments) { o_mom[pix * 2] = m1; o_mom[pix * 2 + 1] = m2; }
            if (t.response) o_lam[pix] = lam;
        }
    f = fopen(argv[11], "wb");
    if (!f) { perror("out"); return 1; }
    fwrite(o_rgba.data(), 4, o_rgba.size(), f); fwrite(o_var.data(), 4, n_px, f); fwrite(o_len.data(), 4, n_px, f);
    if (t.moments) fwrite(o_mom.data(), 4, o_mom.size(), f);
    if (t.response) fwrite(o_lam.data(), 4, n_px, f);
    fclose(f);
    return 0;
}
