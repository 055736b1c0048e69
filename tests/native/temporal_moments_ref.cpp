// CPU checker of the temporal accumulation with luminance moments (csrc/hjr_temporal.hip.h, sections ACCUMULATION, COVERAGE-AWARE ACCUMULATION
// and TEMPORAL MOMENTS of its header comment), restated from that comment as a whole and not derived from the kernel or from the two other
// checkers: fp32, every operation as written, built with -ffp-contract=off so that no multiply-add is fused.
//   temporal_moments_ref W H N_INSTANCES N_TRIANGLES HAVE_PREV PREV_COVERAGE CUR_COVERAGE MOMENTS in.bin out.bin [MOMENTS_MIN]
// in.bin: per side (the previous frame first, if HAVE_PREV; then the current one):  camera (pos, dir, up, right, f: 13 floats) |
//   transforms [n][12] | inverse transforms [n][12] | G-buffer [H][W] 48-byte records | colour [H][W][4] | variance [H][W] | (previous side
//   only) history [H][W] | (previous side only, if MOMENTS) moments [H][W][2].
// out.bin: colour [H][W][4] | variance [H][W] | history [H][W] | (if MOMENTS) moments [H][W][2].
// MOMENTS 0 is the rule without moments (tests/native/temporal_ref.cpp's, or temporal_cov_ref.cpp's with a coverage flag set).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

const float VAR_UNKNOWN = 1e30f, BLEND_ALPHA = 0.2f, SNAP_LIMIT = 0.125f, K_PLANE = 1.0f, K_DIST = 3.0f, H_MAX = 64.0f;
const uint32_t NO_PRIM = 0xffffffffu;

struct Record { uint32_t prim, inst; float t, b1, b2, px, py, pz, nx, ny, nz; uint32_t pad; };
static_assert(sizeof(Record) == 48, "record size");
struct P3 { float x, y, z; };
struct Camera { float pos[3], dir[3], up[3], right[3], f; };
static_assert(sizeof(Camera) == 52, "camera size");

struct Frame {
    Camera cam;
    std::vector<float> fwd, inv, rgba, var, len, mom;
    std::vector<Record> rec;
    bool load(FILE* f, size_t n_inst, size_t n_px, bool is_prev, bool moments)
    {
        fwd.resize(n_inst * 12); inv.resize(n_inst * 12); rec.resize(n_px); rgba.resize(n_px * 4); var.resize(n_px);
        if (fread(&cam, sizeof(cam), 1, f) != 1) return false;
        if (fread(fwd.data(), 4, fwd.size(), f) != fwd.size() || fread(inv.data(), 4, inv.size(), f) != inv.size()) return false;
        if (fread(rec.data(), sizeof(Record), n_px, f) != n_px) return false;
        if (fread(rgba.data(), 4, rgba.size(), f) != rgba.size() || fread(var.data(), 4, n_px, f) != n_px) return false;
        if (!is_prev) return true;
        len.resize(n_px);
        if (fread(len.data(), 4, n_px, f) != n_px) return false;
        if (!moments) return true;
        mom.resize(n_px * 2);
        return fread(mom.data(), 4, mom.size(), f) == mom.size();
    }
};

P3 p3(const float* v) { return P3{ v[0], v[1], v[2] }; }
P3 minus(P3 a, P3 b) { return P3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
float dot3(P3 a, P3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
P3 cross3(P3 a, P3 b) { return P3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
float row_point(const float* r, P3 p) { return ((r[0] * p.x + r[1] * p.y) + r[2] * p.z) + r[3]; }
float row_vector(const float* r, P3 d) { return (r[0] * d.x + r[1] * d.y) + r[2] * d.z; }
P3 xf_point(const float* m, P3 p) { return P3{ row_point(m, p), row_point(m + 4, p), row_point(m + 8, p) }; }
P3 xf_vector(const float* m, P3 d) { return P3{ row_vector(m, d), row_vector(m + 4, d), row_vector(m + 8, d) }; }
bool is_finite(float x) { return std::fabs(x) <= FLT_MAX; }
float max_nan_second(float a, float b) { return a > b ? a : b; } // fmaxf(a, b) for a b that is no NaN: a NaN in a gives b
float min_plain(float a, float b) { return a < b ? a : b; }
bool is_mixed(uint32_t pad)
{
    const uint32_t total = (pad >> 8) & 0xffu;
    return total > 0u && (pad & 0xffu) < total;
}

struct Pixel { float rgba[4], var, len, m1, m2; };

struct Job {
    int w, h;
    uint32_t n_inst, n_tris;
    bool have_prev, prev_cov, cur_cov, moments;
    float moments_min;
    Frame prev, cur;

    // step 3's tests on one candidate tap; `mixed_cur` chooses between rules 2' and 3'
    bool tap_valid(int tx, int ty, const Record& G, bool mixed_cur, P3 p_obj, P3 ng, float nv, float lim_plane, float lim_dist) const
    {
        if (tx < 0 || ty < 0 || tx >= w || ty >= h) return false;
        const Record& T = prev.rec[(size_t)ty * w + tx];
        if (T.prim == NO_PRIM || T.prim >= n_tris || T.inst != G.inst) return false;
        if (prev_cov) {
            if (mixed_cur ? T.pad != G.pad : is_mixed(T.pad)) return false;
        }
        const P3 e = minus(xf_point(&prev.inv[(size_t)T.inst * 12], P3{ T.px, T.py, T.pz }), p_obj);
        const P3 D = xf_vector(&cur.fwd[(size_t)G.inst * 12], e);
        const float nd = dot3(ng, D);
        if (!(nd * nd <= lim_plane)) return false;
        return dot3(D, D) * (nv * nv) <= lim_dist;
    }

    // false: RESTART
    bool accumulate(size_t pix, Pixel& out) const
    {
        const Record& G = cur.rec[pix];
        if (!have_prev || G.prim == NO_PRIM || G.prim >= n_tris || G.inst >= n_inst) return false;
        const float W = (float)w, H = (float)h;
        // 2. reprojection
        const P3 g_pos = P3{ G.px, G.py, G.pz };
        const P3 p_obj = xf_point(&cur.inv[(size_t)G.inst * 12], g_pos);
        const P3 p_prev = xf_point(&prev.fwd[(size_t)G.inst * 12], p_obj);
        const P3 wv = minus(p_prev, p3(prev.cam.pos));
        const P3 a = P3{ prev.cam.dir[0] * prev.cam.f, prev.cam.dir[1] * prev.cam.f, prev.cam.dir[2] * prev.cam.f };
        const P3 b = p3(prev.cam.right), c = p3(prev.cam.up);
        const P3 bc = cross3(b, c);
        const float det = dot3(a, bc);
        const float s = dot3(wv, bc) / det, su = dot3(a, cross3(wv, c)) / det, sv = dot3(a, cross3(b, wv)) / det;
        const float u = su / s, v = sv / s;
        if (!(det != 0.0f && s > 0.0f && is_finite(s) && is_finite(u) && is_finite(v))) return false;
        const float xp = (u * H + W) * 0.5f - 0.5f, yp = (v * H + H) * 0.5f - 0.5f;
        if (!(xp >= -1.0f && xp < W && yp >= -1.0f && yp < H)) return false;
        // the taps
        int tap_x[4], tap_y[4], n_taps;
        float weight[4];
        const bool mixed_cur = cur_cov && is_mixed(G.pad);
        if (mixed_cur) { // 2'
            const float xr = std::floor(xp + 0.5f), yr = std::floor(yp + 0.5f);
            if (!(std::fabs(xp - xr) <= SNAP_LIMIT && std::fabs(yp - yr) <= SNAP_LIMIT)) return false;
            n_taps = 1; tap_x[0] = (int)xr; tap_y[0] = (int)yr; weight[0] = 1.0f;
        } else {
            const float fx = std::floor(xp), fy = std::floor(yp);
            const float tx = xp - fx, ty = yp - fy;
            n_taps = 4;
            for (int k = 0; k < 4; k++) { tap_x[k] = (int)fx + (k & 1); tap_y[k] = (int)fy + (k >> 1); }
            weight[0] = (1.0f - tx) * (1.0f - ty); weight[1] = tx * (1.0f - ty); weight[2] = (1.0f - tx) * ty; weight[3] = tx * ty;
        }
        // 3. what the validity tests share
        const P3 view = minus(g_pos, p3(cur.cam.pos)), ng = P3{ G.nx, G.ny, G.nz };
        const float vv = dot3(view, view), fh = cur.cam.f * H;
        const float fp2 = (vv * 4.0f) / (fh * fh), nn = dot3(ng, ng), nv = dot3(ng, view);
        const float lim_plane = ((K_PLANE * K_PLANE) * fp2) * nn, lim_dist = (((K_DIST * K_DIST) * fp2) * nn) * vv;
        // 4. the sums
        float S = 0.0f, C[3] = { 0.0f, 0.0f, 0.0f }, V = 0.0f, Hs = 0.0f, M1 = 0.0f, M2 = 0.0f;
        bool unknown = false;
        for (int k = 0; k < n_taps; k++) {
            if (!tap_valid(tap_x[k], tap_y[k], G, mixed_cur, p_obj, ng, nv, lim_plane, lim_dist)) continue;
            const size_t tap = (size_t)tap_y[k] * w + tap_x[k];
            const float wk = weight[k], pv = prev.var[tap];
            S = S + wk;
            for (int q = 0; q < 3; q++) C[q] = C[q] + prev.rgba[tap * 4 + q] * wk;
            if (!(pv < VAR_UNKNOWN)) unknown = true;
            V = V + max_nan_second(pv, 0.0f) * wk;
            Hs = Hs + prev.len[tap] * wk;
            if (moments) {
                M1 = M1 + prev.mom[tap * 2] * wk;
                M2 = M2 + prev.mom[tap * 2 + 1] * wk;
            }
        }
        if (!(S > 0.0f)) return false;
        const float v_prev = V / S, h_prev = Hs / S;
        const float hl = min_plain(max_nan_second(h_prev + 1.0f, 1.0f), H_MAX);
        const float al = max_nan_second(1.0f / hl, BLEND_ALPHA);
        for (int q = 0; q < 3; q++) {
            const float cp = C[q] / S;
            out.rgba[q] = cp + (cur.rgba[pix * 4 + q] - cp) * al;
        }
        out.rgba[3] = cur.rgba[pix * 4 + 3];
        const float cv = cur.var[pix];
        if (!(cv < VAR_UNKNOWN)) unknown = true;
        const float om = 1.0f - al;
        out.var = unknown ? VAR_UNKNOWN : (om * om) * v_prev + (al * al) * max_nan_second(cv, 0.0f);
        out.len = hl;
        if (moments) {
            const float l = (cur.rgba[pix * 4] + cur.rgba[pix * 4 + 1]) + cur.rgba[pix * 4 + 2];
            const float m1p = M1 / S, m2p = M2 / S;
            out.m1 = m1p + (l - m1p) * al;
            out.m2 = m2p + (l * l - m2p) * al;
            if (hl >= moments_min) {
                const float k = max_nan_second(1.0f / hl, BLEND_ALPHA / (2.0f - BLEND_ALPHA));
                const float d = out.m2 - out.m1 * out.m1;
                float mv = VAR_UNKNOWN;
                if (is_finite(d)) mv = max_nan_second(d, 0.0f) * (k / (1.0f - k));
                out.var = mv < VAR_UNKNOWN ? mv : VAR_UNKNOWN;
            }
        }
        return true;
    }
};

} // namespace

int main(int argc, char** argv)
{
    if (argc != 11 && argc != 12) {
        fprintf(stderr, "usage: temporal_moments_ref W H N_INSTANCES N_TRIANGLES HAVE_PREV PREV_COVERAGE CUR_COVERAGE MOMENTS in out [MOMENTS_MIN]\n");
        return 2;
    }
    Job j;
    j.w = atoi(argv[1]); j.h = atoi(argv[2]);
    j.n_inst = (uint32_t)strtoul(argv[3], nullptr, 10); j.n_tris = (uint32_t)strtoul(argv[4], nullptr, 10);
    j.have_prev = atoi(argv[5]) != 0;
    j.prev_cov = j.have_prev && strtoul(argv[6], nullptr, 10) != 0; j.cur_cov = strtoul(argv[7], nullptr, 10) != 0;
    j.moments = atoi(argv[8]) != 0;
    j.moments_min = argc == 12 ? (float)atof(argv[11]) : 4.0f;
    if (j.w <= 0 || j.h <= 0) { fprintf(stderr, "bad size\n"); return 2; }
    const size_t n_px = (size_t)j.w * j.h;
    FILE* f = fopen(argv[9], "rb");
    if (!f) { perror("in"); return 1; }
    const bool ok = (!j.have_prev || j.prev.load(f, j.n_inst, n_px, true, j.moments)) && j.cur.load(f, j.n_inst, n_px, false, false);
    fclose(f);
    if (!ok) { fprintf(stderr, "short input\n"); return 1; }
    std::vector<float> o_rgba(n_px * 4), o_var(n_px), o_len(n_px), o_mom(j.moments ? n_px * 2 : 0);
    for (size_t pix = 0; pix < n_px; pix++) {
        Pixel px;
        if (!j.accumulate(pix, px)) { // RESTART
            for (int q = 0; q < 4; q++) px.rgba[q] = j.cur.rgba[pix * 4 + q];
            px.var = j.cur.var[pix];
            px.len = 1.0f;
            const float l = (px.rgba[0] + px.rgba[1]) + px.rgba[2];
            px.m1 = l; px.m2 = l * l;
        }
        for (int q = 0; q < 4; q++) o_rgba[pix * 4 + q] = px.rgba[q];
        o_var[pix] = px.var; o_len[pix] = px.len;
        if (j.moments) { o_mom[pix * 2] = px.m1; o_mom[pix * 2 + 1] = px.m2; }
    }
    f = fopen(argv[10], "wb");
    if (!f) { perror("out"); return 1; }
    fwrite(o_rgba.data(), 4, o_rgba.size(), f); fwrite(o_var.data(), 4, n_px, f); fwrite(o_len.data(), 4, n_px, f);
    if (j.moments) fwrite(o_mom.data(), 4, o_mom.size(), f);
    fclose(f);
    return 0;
}
