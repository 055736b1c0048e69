// Per-frame BVH4 build on the device (option "device_bvh" = 1): the same frame data host/frame.cpp::build_frame
// emits for the memory layout (lds_mode 0, HJR_NODE4_F4 nodes), from a Morton-order tree instead of binned SAH.
//   flatten      one lane per triangle: world vertices, shading record, instance id, padded box inputs (frame.cpp's expressions)
//   morton       padding from the exact maximum |coordinate|, 63-bit codes over the centroid bounds
//   radix sort   stable LSD over (code, prim id), 8 bits per pass, reduce-then-scan in separate launches
//   hierarchy    Karras 2012: every inner node finds its range and split on its own (ties by index)
//   boxes        bottom-up, one agent-scope acq_rel counter per inner node: the second lane to arrive takes the union
//   treelets     ("device_bvh_opt" rounds) Karras & Aila 2013: bottom-up climbs with the same hand-off, a wave per 7-leaf treelet
//                finds its SAH-optimal topology; then leaf positions and inner ranges are recomputed and tri_geom is gathered in the new order
//   collapse     BVH4 level by level with emit_bvh4's rules; ids from a scan of each level (breadth-first, same bytes every run)
//   cost         BVH4 SAH of the final nodes, summed in a fixed order (the same bits every run); also after a refit
// Refit (option "device_bvh_refit", device_bvh_refit below): new transforms over the CURRENT frame data's topology.  flatten in leaf order
// (the prim id of every tri_geom row), then the node boxes bottom-up over the BVH4 itself with the hand-off of `boxes`; no sort, no hierarchy.
// Instance trees (option "device_bvh_instances", device_bvh_instances below): the BVH2 is built once per scene over object-space boxes with
// the instance id on top of the sort key, so that every instance is one subtree, and kept; a commit flattens in its leaf order, computes
// the world boxes inside the instance subtrees, builds the top tree over the instance boxes in one workgroup, then collapse and cost.
// Grafted instance trees (option "device_bvh_graft" with it): the topology also keeps every instance's BVH4, collapsed once by the
// object-space areas (the skeleton); a commit flattens, refits the skeleton's boxes with the refit's climb, clusters and collapses the
// top tree in one workgroup and places the skeleton behind the top nodes: no per-level launches and no BVH2 after the topology build.
// No workgroup ever waits for another one; every cross-launch size the host does not know is read by the kernels from `hdr`.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/henjou_hip.h"
#include "../host/frame.hpp"
#include "hjr_bvh_build.h"
#include "hjr_layout.h"

namespace {

constexpr int NT = 256;         // threads per workgroup of every kernel here (4 waves)
constexpr int SCAN_G = 256;     // workgroups of the scan passes (== NT: the top pass scans their sums in one workgroup)
constexpr int SORT_TILE = 2048; // keys per workgroup of a radix pass (8 rounds of NT)
constexpr int LEVEL_BATCH = 8;  // collapse levels enqueued between two reads of the frontier size

// header words (uint32)
enum Hdr {
    H_SMAX = 0,      // bits of max |coordinate| over the unpadded triangle boxes (non-negative floats order as their bits)
    H_CMIN = 1,      // 3 ordered-uint centroid minima, then 3 maxima
    H_CMAX = 4,
    H_WORST = 7,     // max pending traversal-stack entries over the wide nodes
    H_DEPTH = 8,     // max BVH2 depth of a wide-node slot
    H_BASE = 9,      // first wide id of the current level
    H_F = 10,        // nodes of the current level
    H_NEXT = 11,     // nodes of the next level (scan total)
    H_ERR = 12,      // non-zero: the restructured BVH2, the BVH4 a refit walks, or the kept instance topology failed a structural bound (reported as HJR_ERR_DEVICE)
    H_SAH = 13,      // float bits: BVH4 SAH of the final nodes (sah_top_kernel)
    H_WORDS = 16
};

__device__ __forceinline__ uint32_t f2o(float f) // order-preserving float -> uint
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float o2f(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
// std::min / std::max of frame.cpp's Box::grow (a NaN operand on the right is dropped, as there)
__device__ __forceinline__ float smin(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float smax(float a, float b) { return a < b ? b : a; }

// exclusive scan over a 256-thread workgroup; `s` holds 4 words of LDS
__device__ uint32_t block_scan(uint32_t v, uint32_t& total, uint32_t* s)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s[w] = x;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
    for (int k = 0; k < NT / 64; k++) { if (k < w) pre += s[k]; tot += s[k]; }
    __syncthreads();
    total = tot;
    return pre + x - v;
}

// ---- generic exclusive scan of n uint32 (n from the host or from a header word), in place allowed: three launches -----------------
__device__ __forceinline__ void scan_range(uint32_t n, uint32_t& b0, uint32_t& b1)
{
    const uint32_t chunk = (n + SCAN_G - 1) / SCAN_G;
    b0 = min(n, blockIdx.x * chunk);
    b1 = min(n, b0 + chunk);
}
__global__ void __launch_bounds__(NT) scan_reduce_kernel(const uint32_t* in, const uint32_t* n_ptr, uint32_t n_const, uint32_t* part)
{
    __shared__ uint32_t s[4];
    const uint32_t n = n_ptr ? *n_ptr : n_const;
    uint32_t b0, b1, acc = 0, tot;
    scan_range(n, b0, b1);
    for (uint32_t i = b0 + threadIdx.x; i < b1; i += NT) acc += in[i];
    block_scan(acc, tot, s);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(NT) scan_top_kernel(uint32_t* part, uint32_t* total)
{
    __shared__ uint32_t s[4];
    uint32_t tot;
    const uint32_t ex = block_scan(part[threadIdx.x], tot, s);
    part[threadIdx.x] = ex;
    if (threadIdx.x == 0 && total) *total = tot;
}
__global__ void __launch_bounds__(NT) scan_down_kernel(const uint32_t* in, uint32_t* out, const uint32_t* n_ptr, uint32_t n_const, const uint32_t* part)
{
    __shared__ uint32_t s[4];
    const uint32_t n = n_ptr ? *n_ptr : n_const;
    uint32_t b0, b1, tot;
    scan_range(n, b0, b1);
    uint32_t run = part[blockIdx.x];
    for (uint32_t base = b0; base < b1; base += NT) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < b1 ? in[i] : 0u;
        const uint32_t ex = block_scan(v, tot, s);
        if (i < b1) out[i] = run + ex;
        run += tot;
    }
}

// ---- morph targets (hjr_set_morph): the working vertex / normal arrays every flatten below reads ---------------------
// One record per set; block_begin: the first workgroup of the set (ascending, set 0 at 0).  pos / nrm: first float of the set's deltas in
// MorphArgs::deltas, target-major (target k of vertex i at 3 * (k * n_vertices + i)), so every target's read is as coalesced as the base's.
struct MorphSetDev { uint32_t first_vertex, n_vertices, n_targets, first_weight, block_begin, has_nrm; unsigned long long pos, nrm; };
struct MorphArgs {
    const float *base_v, *base_n, *deltas, *w;
    const MorphSetDev* sets;
    uint32_t n_sets;
    float *out_v, *out_n;
};
// p = base; p = p + w[k] * d[k] for k = 0 .. K-1, per component: the product rounded, then the sum (this unit is built with -ffp-contract=off).
// The loads of four targets are independent of the sums and issue together; the sums stay in target order.
__device__ __forceinline__ void morph_vertex3(const float* base, const float* d, size_t stride, const float* w, uint32_t K, float* out)
{
    float p0 = base[0], p1 = base[1], p2 = base[2];
#pragma unroll 4
    for (uint32_t k = 0; k < K; k++) {
        const float* dk = d + (size_t)k * stride;
        const float wk = w[k], t0 = wk * dk[0], t1 = wk * dk[1], t2 = wk * dk[2];
        p0 = p0 + t0; p1 = p1 + t1; p2 = p2 + t2;
    }
    out[0] = p0; out[1] = p1; out[2] = p2;
}
// One lane per vertex of a set; a workgroup lies inside one set.  Streaming: no LDS, no scratch, no atomics; every byte is read or written once.
// Vertices outside the sets, and the normals of a set without normal deltas, are not touched: the working arrays hold the base there.
__global__ void __launch_bounds__(NT) hjr_morph_kernel(MorphArgs a)
{
    uint32_t lo = 0, hi = a.n_sets; // the set of this workgroup: the last block_begin <= blockIdx.x (uniform)
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (a.sets[mid].block_begin <= blockIdx.x) lo = mid; else hi = mid; }
    const MorphSetDev s = a.sets[lo];
    const uint32_t i = (blockIdx.x - s.block_begin) * NT + threadIdx.x;
    if (i >= s.n_vertices) return;
    const size_t v = 3 * ((size_t)s.first_vertex + i), stride = 3 * (size_t)s.n_vertices;
    const float* w = a.w + s.first_weight;
    morph_vertex3(a.base_v + v, a.deltas + s.pos + 3 * (size_t)i, stride, w, s.n_targets, a.out_v + v);
    if (s.has_nrm) morph_vertex3(a.base_n + v, a.deltas + s.nrm + 3 * (size_t)i, stride, w, s.n_targets, a.out_n + v);
}

// ---- flatten: frame.cpp:520-543 (world vertices, shading record, instance) and :586-600 (box, centroid, max |coordinate|) ----------
__device__ __forceinline__ void xform_pos(const float* m, float px, float py, float pz, float* o)
{
    o[0] = m[0] * px + m[1] * py + m[2] * pz + m[3] * 1.0f;
    o[1] = m[4] * px + m[5] * py + m[6] * pz + m[7] * 1.0f;
    o[2] = m[8] * px + m[9] * py + m[10] * pz + m[11] * 1.0f;
}
__device__ __forceinline__ void xform_nrm(const float* m, float nx, float ny, float nz, float* o)
{
    o[0] = m[0] * nx + m[4] * ny + m[8] * nz + 0.0f * 0.0f;
    o[1] = m[1] * nx + m[5] * ny + m[9] * nz + 0.0f * 0.0f;
    o[2] = m[2] * nx + m[6] * ny + m[10] * nz + 0.0f * 0.0f;
}

struct FlattenArgs {
    const float *vert, *norm, *uv, *xf;
    const uint32_t *idx, *mat, *prim_off;
    uint32_t n, n_inst;
    float *wv, *shade, *box, *cent; // wv 9 / shade 16 / box 8 (lo xyz -, hi xyz -) / cent 4 floats per triangle
    uint32_t *inst, *hdr;
};

// the instance of triangle t: the last prim_offset <= t (prim_offset[0] == 0)
__device__ __forceinline__ uint32_t instance_of(const FlattenArgs& a, uint32_t t)
{
    uint32_t lo = 0, hi = a.n_inst;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (a.prim_off[mid] <= t) lo = mid; else hi = mid; }
    return lo;
}
// triangle t under its instance's transform: world vertices v[9], shading record s[16]; returns the instance
__device__ __forceinline__ uint32_t flatten_tri(const FlattenArgs& a, uint32_t t, float* v, float* s)
{
    const uint32_t lo = instance_of(a, t);
    const float* m = a.xf + 24 * (size_t)lo;
    const float* mi = m + 12;
    float uv[6];
    for (int k = 0; k < 3; k++) {
        const uint32_t ix = a.idx[3 * (size_t)t + k];
        xform_pos(m, a.vert[3 * (size_t)ix], a.vert[3 * (size_t)ix + 1], a.vert[3 * (size_t)ix + 2], &v[3 * k]);
        float nn[3];
        xform_nrm(mi, a.norm[3 * (size_t)ix], a.norm[3 * (size_t)ix + 1], a.norm[3 * (size_t)ix + 2], nn);
        const float inv = 1.0f / sqrtf(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
        s[4 * k + 0] = nn[0] * inv; s[4 * k + 1] = nn[1] * inv; s[4 * k + 2] = nn[2] * inv;
        uv[2 * k] = a.uv[2 * (size_t)ix]; uv[2 * k + 1] = a.uv[2 * (size_t)ix + 1];
    }
    s[3] = uv[0]; s[7] = uv[1]; s[11] = uv[2];
    s[12] = uv[3]; s[13] = uv[4]; s[14] = uv[5];
    s[15] = __uint_as_float(a.mat[t]);
    return lo;
}
__device__ __forceinline__ void store_shade(float* shade, uint32_t t, const float* s)
{
    float4* sd = reinterpret_cast<float4*>(shade) + 4 * (size_t)t;
    for (int q = 0; q < 4; q++) sd[q] = make_float4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
}
// a tri_geom row (frame.cpp:652-660): the world vertices v[9] of triangle t
__device__ __forceinline__ void store_geom_row(float4* g, const float* v, uint32_t t, uint32_t mat)
{
    g[0] = make_float4(v[0], v[1], v[2], v[3]);
    g[1] = make_float4(v[4], v[5], v[6], v[7]);
    g[2] = make_float4(v[8], __uint_as_float(t), __uint_as_float(mat), 0.0f);
}
// the padding of every leaf box (frame.cpp:603-609) from the finished maximum |coordinate|
__device__ __forceinline__ float frame_pad(const uint32_t* hdr) { return __uint_as_float(hdr[H_SMAX]) * (1.0f / 8192.0f); }
// unpadded box of the triangle; returns its max |coordinate|
__device__ __forceinline__ float tri_box(const float* v, float* bl, float* bh)
{
    float mx = 0.0f;
    for (int ax = 0; ax < 3; ax++) {
        bl[ax] = 3.402823466e+38f; bh[ax] = -3.402823466e+38f;
        for (int k = 0; k < 3; k++) { bl[ax] = smin(bl[ax], v[3 * k + ax]); bh[ax] = smax(bh[ax], v[3 * k + ax]); }
    }
    for (int ax = 0; ax < 3; ax++) mx = smax(mx, smax(fabsf(bl[ax]), fabsf(bh[ax])));
    return mx;
}

__global__ void __launch_bounds__(NT) flatten_kernel(FlattenArgs a)
{
    __shared__ uint32_t s_red[7];
    if (threadIdx.x < 7) s_red[threadIdx.x] = threadIdx.x >= 1 && threadIdx.x < 4 ? 0xffffffffu : 0u;
    __syncthreads();
    const uint32_t t = blockIdx.x * NT + threadIdx.x;
    if (t < a.n) {
        float v[9], s[16];
        const uint32_t lo = flatten_tri(a, t, v, s);
        store_shade(a.shade, t, s);
        for (int k = 0; k < 9; k++) a.wv[9 * (size_t)t + k] = v[k];
        a.inst[t] = lo;
        float bl[3], bh[3], c[3];
        const float mx = tri_box(v, bl, bh);
        for (int ax = 0; ax < 3; ax++) c[ax] = 0.5f * (bl[ax] + bh[ax]);
        float4* bd = reinterpret_cast<float4*>(a.box) + 2 * (size_t)t;
        bd[0] = make_float4(bl[0], bl[1], bl[2], 0.0f);
        bd[1] = make_float4(bh[0], bh[1], bh[2], 0.0f);
        reinterpret_cast<float4*>(a.cent)[t] = make_float4(c[0], c[1], c[2], 0.0f);
        // exact, order-independent reductions: max of non-negative float bits, min / max of order-preserving encodings
        atomicMax(&s_red[0], __float_as_uint(mx));
        for (int ax = 0; ax < 3; ax++) { atomicMin(&s_red[1 + ax], f2o(c[ax])); atomicMax(&s_red[4 + ax], f2o(c[ax])); }
    }
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&a.hdr[H_SMAX], s_red[0]);
    else if (threadIdx.x < 4) atomicMin(&a.hdr[H_CMIN + threadIdx.x - 1], s_red[threadIdx.x]);
    else if (threadIdx.x < 7) atomicMax(&a.hdr[H_CMAX + threadIdx.x - 4], s_red[threadIdx.x]);
}

// ---- padding (frame.cpp:603-609) and Morton codes --------------------------------------------------------------------------
__device__ __forceinline__ uint64_t spread21(uint32_t x) // 21 bits -> every third bit of 63
{
    uint64_t v = x & 0x1fffffull;
    v = (v | (v << 32)) & 0x1f00000000ffffull;
    v = (v | (v << 16)) & 0x1f0000ff0000ffull;
    v = (v | (v << 8)) & 0x100f00f00f00f00full;
    v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}
__device__ __forceinline__ uint32_t quantize21(float c, float lo, float scale)
{
    const float f = (c - lo) * scale;
    return f >= 2097151.0f ? 2097151u : (f > 0.0f ? (uint32_t)f : 0u); // NaN -> 0
}
__global__ void __launch_bounds__(NT) morton_kernel(uint32_t n, float* box, const float* cent, const uint32_t* hdr, uint64_t* keys, uint32_t* vals)
{
    const uint32_t t = blockIdx.x * NT + threadIdx.x;
    if (t >= n) return;
    const float pad = frame_pad(hdr);
    float4* b = reinterpret_cast<float4*>(box) + 2 * (size_t)t;
    float4 lo = b[0], hi = b[1];
    lo.x -= pad; lo.y -= pad; lo.z -= pad;
    hi.x += pad; hi.y += pad; hi.z += pad;
    b[0] = lo; b[1] = hi;
    const float4 c = reinterpret_cast<const float4*>(cent)[t];
    uint64_t key = 0;
    const float cc[3] = { c.x, c.y, c.z };
    for (int ax = 0; ax < 3; ax++) {
        const float l = o2f(hdr[H_CMIN + ax]), h = o2f(hdr[H_CMAX + ax]);
        const float ext = h - l;
        const float scale = ext > 0.0f ? 2097152.0f / ext : 0.0f;
        key |= spread21(quantize21(cc[ax], l, scale)) << (2 - ax);
    }
    keys[t] = key;
    vals[t] = t; // seeded in prim order: the stable sort leaves equal codes in prim-id order
}

// ---- stable LSD radix sort, 8 bits per pass ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) radix_hist_kernel(const uint64_t* keys, uint32_t n, int shift, uint32_t* hist, uint32_t nb)
{
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    for (int r = 0; r < SORT_TILE / NT; r++) {
        const uint32_t i = blockIdx.x * SORT_TILE + r * NT + threadIdx.x;
        if (i < n) atomicAdd(&s_h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nb + blockIdx.x] = s_h[threadIdx.x];
}
// hist: exclusive offsets, digit-major ([digit][workgroup]).  Rounds of NT keys in index order; inside a round a wave ranks its lanes
// among equal digits with eight ballots, the waves are ordered through LDS: the scatter keeps the input order of equal digits.
__global__ void __launch_bounds__(NT) radix_scatter_kernel(const uint64_t* keys, const uint32_t* vals, uint32_t n, int shift, const uint32_t* hist,
                                                           uint32_t nb, uint64_t* keys_out, uint32_t* vals_out)
{
    __shared__ uint32_t s_base[256], s_wc[4][256], s_tot[256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    s_base[threadIdx.x] = hist[(size_t)threadIdx.x * nb + blockIdx.x];
    for (int r = 0; r < SORT_TILE / NT; r++) {
        for (int k = 0; k < 4; k++) s_wc[k][threadIdx.x] = 0;
        __syncthreads();
        const uint32_t i = blockIdx.x * SORT_TILE + r * NT + threadIdx.x;
        const bool valid = i < n;
        const uint64_t key = valid ? keys[i] : 0ull;
        const uint32_t val = valid ? vals[i] : 0u;
        const uint32_t d = (uint32_t)(key >> shift) & 255u;
        uint64_t m = __ballot(valid);
        for (int bit = 0; bit < 8; bit++) {
            const uint64_t bb = __ballot((d >> bit) & 1u);
            m &= ((d >> bit) & 1u) ? bb : ~bb;
        }
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (valid && (m >> lane) == 1ull) s_wc[w][d] = (uint32_t)__popcll(m); // the last lane of its digit in this wave
        __syncthreads();
        { // per digit: the waves' prefix (in place) and the round's total
            uint32_t acc = 0;
            for (int k = 0; k < 4; k++) { const uint32_t c = s_wc[k][threadIdx.x]; s_wc[k][threadIdx.x] = acc; acc += c; }
            s_tot[threadIdx.x] = acc;
        }
        __syncthreads();
        const uint32_t dst = s_base[d] + s_wc[w][d] + rank;
        if (valid && dst < n) { // (always: the offsets are a permutation of [0, n))
            keys_out[dst] = key;
            vals_out[dst] = val;
        }
        __syncthreads();
        s_base[threadIdx.x] += s_tot[threadIdx.x];
    }
}

// ---- leaves in sorted order: tri_geom (frame.cpp:652-660) and the leaf boxes ----------------------------------------------------
// Either output may be null.  `pos` (null: the sorted order itself) is the tri_geom row of sorted leaf k after a restructuring.
__global__ void __launch_bounds__(NT) gather_kernel(uint32_t n, const uint32_t* order, const uint32_t* pos, const float* wv, const uint32_t* mat,
                                                    const float* box, float* tri_geom, float* leaf_box)
{
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= n) return;
    const uint32_t t = order[k];
    const uint32_t d = pos ? pos[k] : k;
    if (tri_geom && d < n) store_geom_row(reinterpret_cast<float4*>(tri_geom) + 3 * (size_t)d, wv + 9 * (size_t)t, t, mat[t]);
    if (leaf_box) {
        const float4* b = reinterpret_cast<const float4*>(box) + 2 * (size_t)t;
        float4* lb = reinterpret_cast<float4*>(leaf_box) + 2 * (size_t)k;
        lb[0] = b[0];
        lb[1] = b[1];
    }
}

// ---- hierarchy (Karras 2012) ----------------------------------------------------------------------------------------------------
// BVH2 refs: inner node i -> i, sorted leaf k -> k | REF_LEAF.  Inner node 0 is the root.
constexpr uint32_t REF_LEAF = 0x80000000u;

__device__ __forceinline__ int delta(const uint64_t* keys, int n, int i, int j)
{
    if (j < 0 || j >= n) return -1;
    const uint64_t a = keys[i], b = keys[j];
    return a == b ? 64 + __clz((uint32_t)(i ^ j)) : __clzll((long long)(a ^ b));
}
// parent: [0, n - 1) inner nodes, then [n - 1, 2n - 1) leaves
__global__ void __launch_bounds__(NT) karras_kernel(int n, const uint64_t* keys, uint2* child, uint2* range, uint32_t* parent)
{
    const int i = (int)(blockIdx.x * NT + threadIdx.x);
    if (i >= n - 1) return;
    const int d = delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = delta(keys, n, i, i - d);
    int lmax = 2;
    while (delta(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = delta(keys, n, i, j);
    int s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + min(d, 0);
    const int first = min(i, j), last = max(i, j);
    const uint32_t left = first == gamma ? ((uint32_t)gamma | REF_LEAF) : (uint32_t)gamma;
    const uint32_t right = last == gamma + 1 ? ((uint32_t)(gamma + 1) | REF_LEAF) : (uint32_t)(gamma + 1);
    child[i] = make_uint2(left, right);
    range[i] = make_uint2((uint32_t)first, (uint32_t)(last - first + 1));
    const size_t pl = (left & REF_LEAF) ? (size_t)(n - 1) + (left & ~REF_LEAF) : left, pr = (right & REF_LEAF) ? (size_t)(n - 1) + (right & ~REF_LEAF) : right;
    if (pl < (size_t)(2 * n - 1)) parent[pl] = (uint32_t)i; // (always: gamma + 1 <= n - 1)
    if (pr < (size_t)(2 * n - 1)) parent[pr] = (uint32_t)i;
}

// ---- boxes, bottom-up ---------------------------------------------------------------------------------------------------------------
// One lane per leaf climbs while it is the second to reach a node.  Cross-workgroup hand-off (MI355X_MICROARCH.md, inter-workgroup
// visibility): the lane stores the box of the node it completed, then its agent-scope acq_rel add on the parent's counter releases
// that store (L2 write-back) and, for the second lane, acquires the sibling's (L1 invalidate) before it reads both boxes.
__device__ __forceinline__ void box_of(uint32_t ref, const float4* leaf_box, const float4* inner_box, float4& lo, float4& hi)
{
    const float4* b = (ref & REF_LEAF) ? leaf_box + 2 * (size_t)(ref & ~REF_LEAF) : inner_box + 2 * (size_t)ref;
    lo = b[0];
    hi = b[1];
}
// the union into (lo, hi): exact min / max
__device__ __forceinline__ void box_union(float4& lo, float4& hi, const float4& l1, const float4& h1)
{
    lo = make_float4(smin(lo.x, l1.x), smin(lo.y, l1.y), smin(lo.z, l1.z), 0.0f);
    hi = make_float4(smax(hi.x, h1.x), smax(hi.y, h1.y), smax(hi.z, h1.z), 0.0f);
}
__global__ void __launch_bounds__(NT) boxes_kernel(int n, const uint2* child, const uint32_t* parent, uint32_t* counter, const float4* leaf_box, float4* inner_box)
{
    const int k = (int)(blockIdx.x * NT + threadIdx.x);
    if (k >= n) return;
    uint32_t p = parent[(size_t)(n - 1) + k];
    for (;;) {
        const uint32_t before = __hip_atomic_fetch_add(&counter[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (before == 0) return; // the sibling's lane finishes this node
        const uint2 c = child[p];
        float4 l0, h0, l1, h1;
        box_of(c.x, leaf_box, inner_box, l0, h0);
        box_of(c.y, leaf_box, inner_box, l1, h1);
        box_union(l0, h0, l1, h1);
        inner_box[2 * (size_t)p] = l0;
        inner_box[2 * (size_t)p + 1] = h0;
        if (p == 0) return;
        p = parent[p];
    }
}

// ---- treelet restructuring (option "device_bvh_opt"; Karras & Aila, HPG 2013) ------------------------------------------------------
// Collapse-aware SAH of a BVH2 node: a node of at most leaf_max triangles becomes a BVH4 leaf (is_inner), so it costs Ct * A * N;
// any other node costs Ci * A plus its children.  The constants of the cost model live here only.
constexpr float SAH_CI = 1.2f, SAH_CT = 1.0f;
constexpr uint32_t TREELET = 7;                      // leaves of a treelet: 127 subsets in the dynamic programme, 6 inner nodes
// A topology replaces the treelet only when its cost times this is still below the current cost: strictly lower by more than float
// rounding of the two sums (<= 13 terms) can explain, so that equal-cost alternatives (all boxes equal) never replace the tree.
constexpr float SAH_ACCEPT = 1.0f + 1.0f / 65536.0f;
// subsets of the 7 treelet leaves by size, then value; size k starts at c_size_start[k]
__constant__ uint8_t c_subsets[127] = {
    1, 2, 4, 8, 16, 32, 64, 3, 5, 6, 9, 10, 12, 17, 18, 20, 24, 33, 34, 36, 40, 48, 65, 66, 68, 72, 80, 96, 7, 11, 13, 14, 19, 21, 22, 25, 26, 28,
    35, 37, 38, 41, 42, 44, 49, 50, 52, 56, 67, 69, 70, 73, 74, 76, 81, 82, 84, 88, 97, 98, 100, 104, 112, 15, 23, 27, 29, 30, 39, 43, 45, 46, 51,
    53, 54, 57, 58, 60, 71, 75, 77, 78, 83, 85, 86, 89, 90, 92, 99, 101, 102, 105, 106, 108, 113, 114, 116, 120, 31, 47, 55, 59, 61, 62, 79, 87, 91,
    93, 94, 103, 107, 109, 110, 115, 117, 118, 121, 122, 124, 63, 95, 111, 119, 123, 125, 126, 127 };
__constant__ uint8_t c_size_start[9] = { 0, 0, 7, 28, 63, 98, 119, 126, 127 };

__device__ __forceinline__ float sah_area(const float4& lo, const float4& hi)
{
    const float dx = hi.x - lo.x, dy = hi.y - lo.y, dz = hi.z - lo.z;
    return (dx < 0) ? 0.0f : 2.0f * (dx * dy + dy * dz + dz * dx);
}
__device__ __forceinline__ float sah_cost(float area, uint32_t cnt, uint32_t leaf_max, float children)
{
    return cnt <= leaf_max ? SAH_CT * area * (float)cnt : fmaf(SAH_CI, area, children);
}
// index of a node in `parent`: inner nodes first, then the leaves
__device__ __forceinline__ size_t parent_slot(int n, uint32_t ref) { return (ref & REF_LEAF) ? (size_t)(n - 1) + (ref & ~REF_LEAF) : ref; }
// the i-th (1-based, increasing) non-empty subset of `mask`: the bits of i deposited into its set bits
__device__ __forceinline__ uint32_t deposit(uint32_t i, uint32_t mask)
{
    uint32_t q = 0;
    for (; mask; mask &= mask - 1, i >>= 1)
        if (i & 1u) q |= mask & (0u - mask);
    return q;
}
// orders this wave's LDS accesses across its lanes (the wave runs one treelet while its other waves climb on their own)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct TreeletArgs {
    int n;
    uint32_t leaf_max, gamma; // treelet roots: nodes of at least gamma triangles
    uint2* child;
    uint32_t *parent, *counter, *count; // count: triangles under each inner node
    float* cost;                        // collapse-aware SAH of each inner node
    const float4* leaf_box;
    float4* inner_box;
    const uint32_t* top; // device_bvh_instances: per inner node, 1 above the instance roots: never a treelet root (null: an ordinary build)
};
__device__ __forceinline__ void node_sah(const TreeletArgs& a, uint32_t ref, uint32_t& cnt, float& cost)
{
    if (ref & REF_LEAF) {
        float4 lo, hi;
        box_of(ref, a.leaf_box, a.inner_box, lo, hi);
        cnt = 1;
        cost = sah_cost(sah_area(lo, hi), 1u, a.leaf_max, 0.0f);
    } else {
        cnt = a.count[ref];
        cost = a.cost[ref];
    }
}

struct TreeletLds {                 // one per wave
    float area[128], cost[128];     // per subset of the treelet's leaves: box area, optimal cost
    uint32_t cnt[128], part[128];   // triangles, best split (the part without the subset's lowest leaf)
    float4 lo[8], hi[8];            // treelet leaves: boxes, refs
    uint32_t ref[8];
    uint32_t inner[8], sub[8];      // treelet inner node ids ([0] the root) and the subset each one takes in the new topology
    uint2 kids[8];
};

// One wave restructures the treelet under R; every lane calls it with the same R and the root's current cost, and every lane gets
// the root's cost back.  Nodes under R are complete: their writers' releases reached R's counter before the climbing lane's acquire,
// whose L1 invalidate covers the whole wave.  The stores here drain with the wave's next agent-scope release (s_waitcnt vmcnt is per
// wave), the climbing lane's add on the parent's counter.
__device__ float treelet(const TreeletArgs& a, TreeletLds& L, uint32_t R, float old_cost, int lane)
{
    wave_sync(); // the previous treelet's reads of L are done
    // formation: lane i < 7 holds treelet leaf i, lane j < 6 inner node j; expand the leaf of largest area (ties: lowest slot)
    const uint2 c0 = a.child[R];
    uint32_t ref = lane == 0 ? c0.x : c0.y, inner = R;
    float4 lo, hi;
    box_of(ref, a.leaf_box, a.inner_box, lo, hi);
    float area = sah_area(lo, hi);
    for (int nl = 2; nl < (int)TREELET; nl++) {
        const bool cand = lane < nl && !(ref & REF_LEAF);
        const uint64_t cm = __ballot(cand);
        if (!cm) return old_cost; // (never: R holds at least gamma >= 7 triangles)
        float m = cand ? area : -INFINITY;
        for (int o = 1; o < 8; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
        m = __shfl(m, 0);
        const uint64_t bm = __ballot(cand && area == m);
        const int b = __ffsll((unsigned long long)(bm ? bm : cm)) - 1;
        const uint32_t rb = __shfl(ref, b);
        const uint2 cb = a.child[rb];
        if (lane == nl - 1) inner = rb;
        if (lane == b || lane == nl) {
            ref = lane == b ? cb.x : cb.y;
            box_of(ref, a.leaf_box, a.inner_box, lo, hi);
            area = sah_area(lo, hi);
        }
    }
    if (lane < (int)TREELET) {
        uint32_t cnt;
        float cost;
        node_sah(a, ref, cnt, cost);
        L.lo[lane] = lo; L.hi[lane] = hi; L.ref[lane] = ref;
        L.cnt[1u << lane] = cnt;
        L.cost[1u << lane] = cost;
    }
    if (lane < (int)TREELET - 1) L.inner[lane] = inner;
    wave_sync();
    // subset boxes (exact min / max) and triangle counts
    for (uint32_t s = (uint32_t)lane; s < 128; s += 64) {
        if (!s) continue;
        const int i0 = __ffs(s) - 1;
        float4 bl = L.lo[i0], bh = L.hi[i0];
        uint32_t c = L.cnt[1u << i0];
        for (uint32_t m = s & (s - 1); m; m &= m - 1) {
            const int i = __ffs(m) - 1;
            box_union(bl, bh, L.lo[i], L.hi[i]);
            c += L.cnt[1u << i];
        }
        L.area[s] = sah_area(bl, bh);
        if (s & (s - 1)) L.cnt[s] = c;
    }
    wave_sync();
    // dynamic programme by subset size; g lanes share a subset's 2^(k-1) - 1 splits and reduce (cost, lowest split index)
    for (uint32_t k = 2; k <= TREELET; k++) {
        const uint32_t g = k == 7 ? 64u : (k == 6 ? 8u : (k == 5 ? 2u : 1u));
        const uint32_t first = c_size_start[k], m = c_size_start[k + 1] - first, P = (1u << (k - 1)) - 1u;
        const uint32_t mi = (uint32_t)lane / g, j = (uint32_t)lane % g;
        float best = INFINITY;
        uint32_t bi = 0xffffffffu, s = 0, delta = 0;
        if (mi < m) {
            s = c_subsets[first + mi];
            delta = s & (s - 1); // the split's part without the lowest leaf is a non-empty subset of delta
            for (uint32_t i = 1 + j; i <= P; i += g) {
                const uint32_t q = deposit(i, delta);
                const float c = L.cost[s ^ q] + L.cost[q];
                if (bi == 0xffffffffu || c < best) { best = c; bi = i; }
            }
        }
        for (uint32_t o = 1; o < g; o <<= 1) {
            const float ob = __shfl_xor(best, (int)o);
            const uint32_t oi = __shfl_xor(bi, (int)o);
            if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (mi < m && j == 0) {
            L.part[s] = deposit(bi, delta);
            L.cost[s] = sah_cost(L.area[s], L.cnt[s], a.leaf_max, best);
        }
        wave_sync();
    }
    const float new_cost = L.cost[127];
    if (!(new_cost * SAH_ACCEPT < old_cost)) return old_cost;
    // the new topology breadth-first from the root: inner node h takes id inner[h] and subset sub[h]
    if (lane == 0) {
        L.sub[0] = 127;
        uint32_t tail = 1;
        for (uint32_t h = 0; h < TREELET - 1; h++) {
            const uint32_t s = L.sub[h], r = L.part[s], l = s ^ r;
            uint32_t kl, kr;
            if (!(l & (l - 1))) kl = L.ref[__ffs(l) - 1];
            else { kl = L.inner[tail]; L.sub[tail] = l; tail = min(tail + 1, TREELET - 1); }
            if (!(r & (r - 1))) kr = L.ref[__ffs(r) - 1];
            else { kr = L.inner[tail]; L.sub[tail] = r; tail = min(tail + 1, TREELET - 1); }
            L.kids[h] = make_uint2(kl, kr);
        }
    }
    wave_sync();
    if (lane < (int)TREELET - 1) {
        const uint32_t id = L.inner[lane], s = L.sub[lane];
        const uint2 kd = L.kids[lane];
        const size_t px = parent_slot(a.n, kd.x), py = parent_slot(a.n, kd.y), slots = 2 * (size_t)a.n - 1;
        a.child[id] = kd;
        if (px < slots) a.parent[px] = id; // (always: the refs are the treelet's own)
        if (py < slots) a.parent[py] = id;
        if (lane > 0) { // the root keeps its box and count; its cost goes back to the climbing lane
            const int i0 = __ffs(s) - 1;
            float4 bl = L.lo[i0], bh = L.hi[i0];
            for (uint32_t m = s & (s - 1); m; m &= m - 1) {
                const int i = __ffs(m) - 1;
                box_union(bl, bh, L.lo[i], L.hi[i]);
            }
            a.inner_box[2 * (size_t)id] = bl;
            a.inner_box[2 * (size_t)id + 1] = bh;
            a.count[id] = L.cnt[s];
            a.cost[id] = L.cost[s];
        }
    }
    return new_cost;
}

// One restructuring round: boxes_kernel's climb (one lane per leaf, the second lane to reach a node continues; nothing waits) computes
// every inner node's count and cost, and a node of at least gamma triangles (under device_bvh_instances: whose leaves lie in one
// instance, so that no treelet rewires across an instance boundary) is a treelet root.  The wave takes its lanes' roots one
// after the other, all 64 lanes in each, and no lane leaves the loop before the wave is done.  A treelet only rewires nodes under its
// root, which are complete, so the result is the same whatever order the lanes run in.
__global__ void __launch_bounds__(NT) treelet_kernel(TreeletArgs a)
{
    __shared__ TreeletLds s_tl[NT / 64];
    TreeletLds& L = s_tl[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    const int k = (int)(blockIdx.x * NT + threadIdx.x);
    bool active = k < a.n;
    uint32_t p = active ? a.parent[(size_t)(a.n - 1) + k] : 0u;
    while (__ballot(active)) {
        bool done = false; // this lane completed node p
        uint32_t cnt = 0;
        float cost = 0.0f;
        if (active) {
            const uint32_t before = __hip_atomic_fetch_add(&a.counter[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (before == 0) active = false; // the sibling's lane finishes this node
            else {
                const uint2 c = a.child[p];
                uint32_t n0, n1;
                float c0, c1;
                node_sah(a, c.x, n0, c0);
                node_sah(a, c.y, n1, c1);
                float4 lo, hi;
                box_of(p, a.leaf_box, a.inner_box, lo, hi);
                cnt = n0 + n1;
                cost = sah_cost(sah_area(lo, hi), cnt, a.leaf_max, c0 + c1);
                done = true;
            }
        }
        for (uint64_t roots = __ballot(done && cnt >= a.gamma && !(a.top && a.top[p])); roots; roots &= roots - 1) {
            const int src = __ffsll((unsigned long long)roots) - 1;
            const float nc = treelet(a, L, __shfl(p, src), __shfl(cost, src), lane);
            if (lane == src) cost = nc;
        }
        if (done) {
            a.count[p] = cnt;
            a.cost[p] = cost;
            if (p == 0) active = false;
            else p = a.parent[p];
        }
    }
}

// ---- re-layout after restructuring: subtrees are no longer ranges of the sorted order ------------------------------------------
// Leaf k's tri_geom row: the triangles left of it in a depth-first, left-before-right walk (the counts of the left siblings on its
// path to the root).  Bounded by n steps; a longer path or an out-of-range parent sets H_ERR.
__global__ void __launch_bounds__(NT) leaf_pos_kernel(int n, const uint2* child, const uint32_t* parent, const uint32_t* count, uint32_t* pos, uint32_t* hdr)
{
    const int k = (int)(blockIdx.x * NT + threadIdx.x);
    if (k >= n) return;
    uint32_t ref = (uint32_t)k | REF_LEAF, at = 0;
    for (int steps = 0; ref != 0; steps++) { // inner node 0 is the root
        const uint32_t p = parent[parent_slot(n, ref)];
        if (steps >= n || p >= (uint32_t)(n - 1)) { atomicOr(&hdr[H_ERR], 1u); at = 0; break; }
        const uint2 c = child[p];
        if (c.y == ref) at += (c.x & REF_LEAF) ? 1u : (c.x < (uint32_t)(n - 1) ? count[c.x] : 0u);
        ref = p;
    }
    pos[k] = at;
}
// (first, count) of every inner node: the row of its leftmost leaf and its triangle count, what is_inner and wide_emit_kernel read
__global__ void __launch_bounds__(NT) inner_range_kernel(int n, const uint2* child, const uint32_t* count, const uint32_t* pos, uint2* range, uint32_t* hdr)
{
    const int i = (int)(blockIdx.x * NT + threadIdx.x);
    if (i >= n - 1) return;
    uint32_t r = (uint32_t)i;
    for (int steps = 0; !(r & REF_LEAF); steps++) {
        if (steps >= n || r >= (uint32_t)(n - 1)) { atomicOr(&hdr[H_ERR], 2u); r = REF_LEAF; break; }
        r = child[r].x;
    }
    const uint32_t leaf = r & ~REF_LEAF;
    if (leaf >= (uint32_t)n) atomicOr(&hdr[H_ERR], 2u);
    range[i] = make_uint2(leaf < (uint32_t)n ? pos[leaf] : 0u, count[i]);
}

// ---- collapse to BVH4 (frame.cpp::emit_bvh4) ------------------------------------------------------------------------------------
struct Front { uint32_t ref, pend, depth, tag; };     // a wide node of the current level: its BVH2 node, pending entries above it, its depth, its instance (skeleton; else 0)
struct Wide { uint32_t child[4], depth[4], n, pend, tag, pad; }; // children in emit_bvh4's slot order

struct CollapseArgs {
    const uint2 *child, *range;
    const float4 *leaf_box, *inner_box;
    const uint32_t* leaf_pos; // tri_geom row of each sorted leaf after a restructuring (null: the sorted order)
    uint32_t leaf_max;
    uint32_t cap; // wide nodes the buffers hold (>= the wide nodes of any tree over these triangles)
    uint32_t* hdr;
    const uint32_t* top; // device_bvh_instances: per inner node, 1 above the instance roots (null: an ordinary build)
    uint32_t* inst_stat; // device_bvh_graft, the skeleton: per instance (Front::tag) the maxima of h and of the leaf depth (null otherwise)
};
// a BVH2 node that becomes a wide node: inner, and the root or more than leaf_max triangles (frame.cpp:166).  A node above the
// instance roots always does: instances keep their id order in tri_geom, so its triangles are no contiguous row range.
__device__ __forceinline__ bool is_inner(const CollapseArgs& a, uint32_t ref)
{
    return !(ref & REF_LEAF) && (ref == 0 || (a.top && a.top[ref]) || a.range[ref].y > a.leaf_max);
}
// unused slot of a node: inverted box, empty leaf
constexpr float EMPTY_LO = 1e30f, EMPTY_HI = -1e30f;
__host__ __device__ inline void empty_slot(float* q, int c)
{
    for (int ax = 0; ax < 3; ax++) { q[8 * ax + c] = EMPTY_LO; q[8 * ax + 4 + c] = EMPTY_HI; }
    q[24 + c] = __builtin_bit_cast(float, (uint32_t)HJR_LEAF_FLAG);
}
// q[28]: six rows of slot bounds (lo x, hi x, lo y, ...) and the refs row -> the node's seven float4
__device__ __forceinline__ void store_node(float4* o, const float* q)
{
    for (int v = 0; v < HJR_NODE4_F4; v++) o[v] = make_float4(q[4 * v], q[4 * v + 1], q[4 * v + 2], q[4 * v + 3]);
}
__global__ void __launch_bounds__(NT) wide_expand_kernel(CollapseArgs a, const Front* fr, Wide* wide, uint32_t* n_inner)
{
    const uint32_t F = a.hdr[H_F];
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < F && i < a.cap; i += gridDim.x * NT) {
        const Front f = fr[i];
        Wide w;
        w.n = 0;
        if (!is_inner(a, f.ref)) { w.child[0] = f.ref; w.depth[0] = f.depth; w.n = 1; } // a single leaf: wide root with one leaf child
        else {
            const uint2 c = a.child[f.ref];
            w.child[0] = c.x; w.child[1] = c.y; w.depth[0] = w.depth[1] = f.depth + 1; w.n = 2;
        }
        while (w.n < 4) { // replace the largest-area inner child by its two children
            int best = -1;
            float barea = -1.0f;
            for (uint32_t k = 0; k < w.n; k++)
                if (is_inner(a, w.child[k])) {
                    float4 lo, hi;
                    box_of(w.child[k], a.leaf_box, a.inner_box, lo, hi);
                    const float ar = sah_area(lo, hi);
                    if (ar > barea) { barea = ar; best = (int)k; }
                }
            if (best < 0) break;
            const uint2 c = a.child[w.child[best]];
            const uint32_t dd = w.depth[best] + 1;
            w.child[best] = c.x; w.depth[best] = dd;
            w.child[w.n] = c.y; w.depth[w.n] = dd; w.n++;
        }
        uint32_t ni = 0;
        for (uint32_t k = 0; k < w.n; k++) ni += is_inner(a, w.child[k]) ? 1u : 0u;
        w.pend = f.pend;
        w.tag = f.tag;
        w.pad = 0u;
        wide[i] = w;
        n_inner[i] = ni;
    }
}
// writes the level's nodes (ids H_BASE + i) and the next level's frontier (ids H_BASE + F + off[i] + k)
__global__ void __launch_bounds__(NT) wide_emit_kernel(CollapseArgs a, const Wide* wide, const uint32_t* off, Front* next, float4* nodes)
{
    const uint32_t F = a.hdr[H_F], base = a.hdr[H_BASE];
    uint32_t worst = 0, depth = 0;
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < F && base + i < a.cap; i += gridDim.x * NT) {
        const Wide w = wide[i];
        float q[28];
        uint32_t k_in = 0;
        // emit_bvh4's stack bound: a visited wide node leaves (children - 1) entries pending above those of its parent
        const uint32_t h = w.pend + (w.n > 0 ? w.n - 1 : 0);
        worst = max(worst, h);
        uint32_t leaf_depth = 0;
        for (int c = 0; c < 4; c++) {
            if ((uint32_t)c < w.n) {
                const uint32_t r = w.child[c];
                float4 lo, hi;
                box_of(r, a.leaf_box, a.inner_box, lo, hi);
                q[c] = lo.x; q[4 + c] = hi.x; q[8 + c] = lo.y; q[12 + c] = hi.y; q[16 + c] = lo.z; q[20 + c] = hi.z;
                uint32_t ref;
                if (is_inner(a, r)) {
                    const uint32_t j = off[i] + k_in++;
                    ref = base + F + j;
                    if (j < a.cap) next[j] = Front{ r, h, w.depth[c], w.tag };
                } else {
                    ref = (r & REF_LEAF) ? (HJR_LEAF_FLAG | (1u << 27) | (a.leaf_pos ? a.leaf_pos[r & ~REF_LEAF] : (r & ~REF_LEAF))) : (HJR_LEAF_FLAG | (a.range[r].y << 27) | a.range[r].x);
                    leaf_depth = max(leaf_depth, w.depth[c]);
                }
                q[24 + c] = __uint_as_float(ref);
            } else empty_slot(q, c);
        }
        depth = max(depth, leaf_depth);
        if (a.inst_stat) { // integer maxima: the same values whatever order the lanes run in
            atomicMax(&a.inst_stat[2 * (size_t)w.tag], h);
            atomicMax(&a.inst_stat[2 * (size_t)w.tag + 1], leaf_depth);
        }
        store_node(nodes + (size_t)(base + i) * HJR_NODE4_F4, q);
    }
    if (worst) atomicMax(&a.hdr[H_WORST], worst);
    if (depth) atomicMax(&a.hdr[H_DEPTH], depth);
}
__global__ void level_advance_kernel(uint32_t* hdr)
{
    hdr[H_BASE] += hdr[H_F];
    hdr[H_F] = hdr[H_NEXT];
}
__global__ void collapse_init_kernel(uint32_t n, Front* fr, uint32_t* hdr)
{
    fr[0] = Front{ n == 1 ? REF_LEAF : 0u, 0u, 0u, 0u };
    hdr[H_BASE] = 0;
    hdr[H_F] = 1;
}
__global__ void set_word_kernel(uint32_t* w, uint32_t v) { *w = v; }
__global__ void hdr_init_kernel(uint32_t* hdr)
{
    if (threadIdx.x < H_WORDS) hdr[threadIdx.x] = threadIdx.x >= H_CMIN && threadIdx.x < H_CMAX ? 0xffffffffu : 0u;
}

// ---- tree cost: BVH4 SAH of the final nodes (tools/device_bvh_bench.py::bvh4_sah) -------------------------------------------------
// Ci per inner slot, Ct per triangle of a leaf slot, by slot area; sah_top_kernel divides by the root's area.  fp32 in a fixed order:
// a lane adds its nodes' terms in index order, then block_sum's tree, then the SCAN_G partial sums through the same tree.  No float
// atomics: the value has the same bits on every run and after a build and a refit that wrote the same nodes.
__device__ __forceinline__ float slot_area(float lx, float hx, float ly, float hy, float lz, float hz)
{
    const float dx = fmaxf(hx - lx, 0.0f), dy = fmaxf(hy - ly, 0.0f), dz = fmaxf(hz - lz, 0.0f);
    return 2.0f * (dx * dy + dy * dz + dz * dx);
}
__device__ __forceinline__ uint32_t ref_of(const float4& r, int c)
{
    return __float_as_uint(c == 0 ? r.x : (c == 1 ? r.y : (c == 2 ? r.z : r.w)));
}
__device__ __forceinline__ float f4_at(const float4& r, int c) { return c == 0 ? r.x : (c == 1 ? r.y : (c == 2 ? r.z : r.w)); }
__device__ __forceinline__ bool ref_inner(uint32_t ref) { return !(ref & HJR_LEAF_FLAG); }
__device__ __forceinline__ uint32_t inner_slots(const float4& r)
{
    return (ref_inner(__float_as_uint(r.x)) ? 1u : 0u) + (ref_inner(__float_as_uint(r.y)) ? 1u : 0u) + (ref_inner(__float_as_uint(r.z)) ? 1u : 0u) +
           (ref_inner(__float_as_uint(r.w)) ? 1u : 0u);
}
__device__ __forceinline__ float node_sah_term(const float4* nd)
{
    const float4 r = nd[6];
    float term = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint32_t ref = ref_of(r, c);
        if (ref == HJR_LEAF_FLAG) continue;
        const float w = ref_inner(ref) ? SAH_CI : SAH_CT * (float)((ref >> 27) & 15u);
        term += w * slot_area(f4_at(nd[0], c), f4_at(nd[1], c), f4_at(nd[2], c), f4_at(nd[3], c), f4_at(nd[4], c), f4_at(nd[5], c));
    }
    return term;
}
// sum over a 256-thread workgroup in a fixed tree; `s` holds 4 floats of LDS
__device__ float block_sum(float v, float* s)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = (s[0] + s[1]) + (s[2] + s[3]);
    __syncthreads();
    return t;
}
// `counter` (refit only, else null): a node whose inner children did not all arrive was never written -> H_ERR
__global__ void __launch_bounds__(NT) sah_reduce_kernel(const float4* nodes, const uint32_t* n_ptr, uint32_t cap, const uint32_t* counter, float* part, uint32_t* hdr)
{
    __shared__ float s[4];
    const uint32_t n = min(*n_ptr, cap);
    uint32_t b0, b1;
    scan_range(n, b0, b1);
    float acc = 0.0f;
    bool bad = false;
    for (uint32_t i = b0 + threadIdx.x; i < b1; i += NT) {
        const float4* nd = nodes + (size_t)i * HJR_NODE4_F4;
        acc += node_sah_term(nd);
        if (counter && counter[i] != inner_slots(nd[6])) bad = true;
    }
    if (bad) atomicOr(&hdr[H_ERR], 64u);
    const float tot = block_sum(acc, s);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(NT) sah_top_kernel(const float4* nodes, const float* part, uint32_t* hdr)
{
    __shared__ float s[4];
    const float tot = block_sum(part[threadIdx.x], s);
    if (threadIdx.x == 0) {
        float lo[3] = { 1e30f, 1e30f, 1e30f }, hi[3] = { -1e30f, -1e30f, -1e30f };
        for (int c = 0; c < 4; c++) {
            if (ref_of(nodes[6], c) == HJR_LEAF_FLAG) continue;
            for (int ax = 0; ax < 3; ax++) { lo[ax] = smin(lo[ax], f4_at(nodes[2 * ax], c)); hi[ax] = smax(hi[ax], f4_at(nodes[2 * ax + 1], c)); }
        }
        const float ra = slot_area(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]);
        hdr[H_SAH] = __float_as_uint(ra > 0.0f ? tot / ra : 0.0f);
    }
}

// ---- leaf-order flatten, parent pass and node-box climb over a BVH4: the refit, the instance trees and the grafted skeleton -------
// Every index read from kept data (the current frame data, the kept topology) is checked before it is used; a violated bound sets an
// H_ERR bit and the commit fails.
struct LeafFlattenArgs {
    FlattenArgs f;               // scene, transforms, shade / inst / hdr (wv, box, cent unused)
    const float4* cur_geom;      // the refit: row d takes the triangle the current row d holds (its prim id) ...
    const uint32_t *order, *pos; // ... or (cur_geom null) the kept leaf order: sorted leaf k holds triangle order[k] in tri_geom row pos[k]
    float4* geom;                // the builder's tri_geom
    float4* leaf_box;            // per leaf k its unpadded world box (null: the node boxes come from tri_geom)
};
__global__ void __launch_bounds__(NT) leaf_flatten_kernel(LeafFlattenArgs a)
{
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k < a.f.n) {
        const uint32_t t = a.cur_geom ? __float_as_uint(a.cur_geom[HJR_TRI_F4 * (size_t)k + 2].y) : a.order[k];
        const uint32_t d = a.cur_geom ? k : a.pos[k];
        if (t >= a.f.n || d >= a.f.n) atomicOr(&a.f.hdr[H_ERR], 4u);
        else {
            float v[9], s[16], bl[3], bh[3];
            const uint32_t inst = flatten_tri(a.f, t, v, s);
            store_shade(a.f.shade, t, s);
            a.f.inst[t] = inst;
            store_geom_row(a.geom + HJR_TRI_F4 * (size_t)d, v, t, a.f.mat[t]);
            atomicMax(&s_max, __float_as_uint(tri_box(v, bl, bh)));
            if (a.leaf_box) {
                a.leaf_box[2 * (size_t)k] = make_float4(bl[0], bl[1], bl[2], 0.0f);
                a.leaf_box[2 * (size_t)k + 1] = make_float4(bh[0], bh[1], bh[2], 0.0f);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&a.f.hdr[H_SMAX], s_max);
}
// 4 * parent + slot of every node an inner slot refers to, from the refs rows refs[i * stride]: ids are breadth-first, so a child's id
// is above its parent's.  `n_tris` (0: unchecked) bounds the leaf refs; `keep` (or null) takes a copy of the refs rows.
__global__ void __launch_bounds__(NT) node_parent_kernel(uint32_t n_nodes, const float4* refs, uint32_t stride, uint32_t n_tris, float4* keep, uint32_t* parent,
                                                         uint32_t* hdr)
{
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i >= n_nodes) return;
    const float4 r = refs[(size_t)i * stride];
    if (keep) keep[i] = r;
    uint32_t err = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint32_t ref = ref_of(r, c);
        if (ref_inner(ref)) {
            if (ref <= i || ref >= n_nodes) err |= 8u;
            else parent[ref] = 4u * i + (uint32_t)c;
        } else if (n_tris && (ref & 0x7ffffffu) + ((ref >> 27) & 15u) > n_tris) err |= 16u;
    }
    if (err) atomicOr(&hdr[H_ERR], err);
}
// the box of a node's four slots; an unused slot (EMPTY_LO / EMPTY_HI) changes no min / max
__device__ __forceinline__ void slots_box(const float4* nd, float* lo, float* hi)
{
    for (int ax = 0; ax < 3; ax++) {
        const float4 l = nd[2 * ax], h = nd[2 * ax + 1];
        lo[ax] = smin(smin(l.x, l.y), smin(l.z, l.w));
        hi[ax] = smax(smax(h.x, h.y), smax(h.z, h.w));
    }
}
// the padded box of the cnt > 0 tri_geom rows from `first`
__device__ __forceinline__ void rows_box(const float4* geom, uint32_t first, uint32_t cnt, float pad, float* lo, float* hi)
{
    for (int ax = 0; ax < 3; ax++) { lo[ax] = 3.402823466e+38f; hi[ax] = -3.402823466e+38f; }
    for (uint32_t k = 0; k < cnt; k++) {
        const float4* g = geom + HJR_TRI_F4 * (size_t)(first + k);
        const float4 g0 = g[0], g1 = g[1], g2 = g[2];
        lo[0] = smin(smin(lo[0], g0.x), smin(g0.w, g1.z)); hi[0] = smax(smax(hi[0], g0.x), smax(g0.w, g1.z));
        lo[1] = smin(smin(lo[1], g0.y), smin(g1.x, g1.w)); hi[1] = smax(smax(hi[1], g0.y), smax(g1.x, g1.w));
        lo[2] = smin(smin(lo[2], g0.z), smin(g1.y, g2.x)); hi[2] = smax(smax(hi[2], g0.z), smax(g1.y, g2.x));
    }
    for (int ax = 0; ax < 3; ax++) { lo[ax] -= pad; hi[ax] += pad; }
}
struct NodeBoxArgs {
    uint32_t n, n_nodes;     // triangles, nodes
    const float4* refs;      // the refs row of node i is refs[i * stride]: the current nodes (stride HJR_NODE4_F4, from row 6) or the kept rows (1)
    uint32_t stride;
    bool forest;             // the skeleton: a climb ends at a node whose parent word is SK_NONE (else at node 0)
    const float4* geom;      // this commit's tri_geom
    float4* nodes;           // the output, n_nodes nodes
    const uint32_t* parent;  // per node: 4 * parent + slot
    uint32_t *counter, *hdr; // per node: inner children that have arrived
};
constexpr uint32_t SK_NONE = 0xffffffffu;
// writes node i of the output: refs unchanged, leaf slots from the new triangles, inner slots from the child nodes already written
__device__ __forceinline__ void refit_node(const NodeBoxArgs& a, uint32_t i, const float4& r, float pad)
{
    float q[24];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint32_t ref = ref_of(r, c);
        float lo[3] = { EMPTY_LO, EMPTY_LO, EMPTY_LO }, hi[3] = { EMPTY_HI, EMPTY_HI, EMPTY_HI };
        if (ref_inner(ref)) {
            if (ref > i && ref < a.n_nodes) slots_box(a.nodes + (size_t)ref * HJR_NODE4_F4, lo, hi);
        } else if (ref != HJR_LEAF_FLAG) {
            const uint32_t first = ref & 0x7ffffffu, cnt = (ref >> 27) & 15u;
            if (first + cnt <= a.n && cnt > 0) rows_box(a.geom, first, cnt, pad, lo, hi);
        }
        for (int ax = 0; ax < 3; ax++) { q[8 * ax + c] = lo[ax]; q[8 * ax + 4 + c] = hi[ax]; }
    }
    float4* o = a.nodes + (size_t)i * HJR_NODE4_F4;
    for (int v = 0; v < 6; v++) o[v] = make_float4(q[4 * v], q[4 * v + 1], q[4 * v + 2], q[4 * v + 3]);
    o[6] = r;
}
// One lane per node without inner children starts there and climbs while it is the last inner child to reach the parent: boxes_kernel's
// hand-off.  The lane stores the node it finished, then its agent-scope acq_rel add on the parent's counter releases those stores and,
// for the last arriver, acquires the siblings' before it reads their nodes.  refit_node checks every ref before it follows it and a
// parent id must be below the child's, so every climb ends; a node whose children did not all arrive is found by the tree cost (the
// refit) or by graft_place_kernel (the skeleton, whose output is the stage at the skeleton ids).
__global__ void __launch_bounds__(NT) node_boxes_kernel(NodeBoxArgs a)
{
    uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i >= a.n_nodes) return;
    float4 r = a.refs[(size_t)i * a.stride];
    if (inner_slots(r) != 0) return;
    const float pad = frame_pad(a.hdr);
    for (;;) {
        refit_node(a, i, r, pad);
        if (!a.forest && i == 0) return;
        const uint32_t ps = a.parent[i];
        if (a.forest && ps == SK_NONE) return; // an instance root
        const uint32_t p = ps >> 2;
        if (p >= i) { atomicOr(&a.hdr[H_ERR], 32u); return; } // not the parent pass's value: no slot refers to this node
        r = a.refs[(size_t)p * a.stride];
        const uint32_t before = __hip_atomic_fetch_add(&a.counter[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (before + 1u != inner_slots(r)) return; // a sibling's lane finishes the parent
        i = p;
    }
}

// ---- instance trees (option "device_bvh_instances") ---------------------------------------------------------------------------------
// Topology, once per uploaded scene and build tag: the builder's own passes over object-space boxes, with the instance id in the top
// bits of the sort key.  Keys that share a prefix form one subtree of a binary radix tree, so every instance is one contiguous range of
// the sorted order and one subtree; the k - 1 `top` nodes above the instance roots are a radix tree over instance ids, spatially
// meaningless: storage for the top tree every commit builds.  No transform enters the topology.
// Every commit: flatten in leaf order, boxes bottom-up inside the instance subtrees, the top tree, then the build's collapse and cost.
// H_ERR bits of these kernels: 4 leaf order, 128 top-node list, 256 subtree walk, 512 instance roots, 1024 top tree.
__global__ void __launch_bounds__(NT) obj_box_kernel(FlattenArgs a, uint32_t* bmin, uint32_t* bmax)
{
    const uint32_t t = blockIdx.x * NT + threadIdx.x;
    if (t >= a.n) return;
    const uint32_t lo = instance_of(a, t);
    float v[9], bl[3], bh[3];
    for (int k = 0; k < 3; k++) {
        const uint32_t ix = a.idx[3 * (size_t)t + k];
        for (int ax = 0; ax < 3; ax++) v[3 * k + ax] = a.vert[3 * (size_t)ix + ax];
    }
    (void)tri_box(v, bl, bh);
    float4* bd = reinterpret_cast<float4*>(a.box) + 2 * (size_t)t;
    bd[0] = make_float4(bl[0], bl[1], bl[2], 0.0f);
    bd[1] = make_float4(bh[0], bh[1], bh[2], 0.0f);
    a.inst[t] = lo;
    float c[3];
    for (int ax = 0; ax < 3; ax++) c[ax] = 0.5f * (bl[ax] + bh[ax]);
    reinterpret_cast<float4*>(a.cent)[t] = make_float4(c[0], c[1], c[2], 0.0f);
    // exact, order-independent bounds per instance.  The words only ever move outwards, so a stale plain read shows a tighter
    // bound than the current one: an atomic it lets through is redundant at worst, and one it skips would not have changed the word
    for (int ax = 0; ax < 3; ax++) {
        const uint32_t o = f2o(c[ax]);
        if (o < bmin[3 * (size_t)lo + ax]) atomicMin(&bmin[3 * (size_t)lo + ax], o);
        if (o > bmax[3 * (size_t)lo + ax]) atomicMax(&bmax[3 * (size_t)lo + ax], o);
    }
}
// key: instance id in the top `bits` bits of 63, the Morton code over the instance's own centroid bounds (its top 63 - bits bits) below
__global__ void __launch_bounds__(NT) obj_morton_kernel(uint32_t n, const float* cent, const uint32_t* inst, const uint32_t* bmin, const uint32_t* bmax, int bits,
                                                        uint64_t* keys, uint32_t* vals)
{
    const uint32_t t = blockIdx.x * NT + threadIdx.x;
    if (t >= n) return;
    const uint32_t in = inst[t];
    const float4 c = reinterpret_cast<const float4*>(cent)[t];
    const float cc[3] = { c.x, c.y, c.z };
    uint64_t key = 0;
    for (int ax = 0; ax < 3; ax++) {
        const float l = o2f(bmin[3 * (size_t)in + ax]), h = o2f(bmax[3 * (size_t)in + ax]);
        const float ext = h - l;
        const float scale = ext > 0.0f ? 2097152.0f / ext : 0.0f;
        key |= spread21(quantize21(cc[ax], l, scale)) << (2 - ax);
    }
    keys[t] = bits ? (((uint64_t)in << (63 - bits)) | (key >> bits)) : key;
    vals[t] = t;
}
// top[i]: inner node i's leaves (its Karras range of the sorted order) lie in more than one instance
__global__ void __launch_bounds__(NT) top_flag_kernel(int n, const uint64_t* keys, const uint2* range, int shift, uint32_t* top)
{
    const int i = (int)(blockIdx.x * NT + threadIdx.x);
    if (i >= n - 1) return;
    const uint2 r = range[i];
    const uint32_t last = min(r.x + r.y - 1u, (uint32_t)(n - 1));
    top[i] = r.x < (uint32_t)n && (keys[r.x] >> shift) != (keys[last] >> shift) ? 1u : 0u;
}
// root[instance]: the node (or single leaf) that is not a top node and has none but top nodes above it
__global__ void __launch_bounds__(NT) inst_root_kernel(int n, uint32_t n_inst, const uint64_t* keys, const uint2* range, const uint32_t* parent, const uint32_t* top,
                                                       int shift, uint32_t* root, uint32_t* hdr)
{
    const uint32_t s = blockIdx.x * NT + threadIdx.x;
    if (s >= 2u * (uint32_t)n - 1u) return;
    const bool inner = s < (uint32_t)(n - 1);
    if (inner && top[s]) return;
    if (n >= 2 && s != 0) {
        const uint32_t p = parent[s];
        if (p >= (uint32_t)(n - 1)) { atomicOr(&hdr[H_ERR], 512u); return; }
        if (!top[p]) return;
    }
    const uint32_t leaf = inner ? range[s].x : s - (uint32_t)(n - 1);
    const uint64_t in = leaf < (uint32_t)n ? keys[leaf] >> shift : ~0ull;
    if (in >= n_inst) { atomicOr(&hdr[H_ERR], 512u); return; }
    root[in] = inner ? s : (REF_LEAF | leaf);
}
// ids of the top nodes in ascending order (one workgroup); there are k - 1 of them and the first is the root
__global__ void __launch_bounds__(NT) top_ids_kernel(uint32_t n_inner, const uint32_t* top, uint32_t k, uint32_t* ids, uint32_t* hdr)
{
    __shared__ uint32_t s[4];
    uint32_t run = 0, tot;
    for (uint32_t base = 0; base < n_inner; base += NT) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t f = i < n_inner && top[i] ? 1u : 0u;
        const uint32_t at = run + block_scan(f, tot, s);
        if (f && at + 1 < k) ids[at] = i;
        run += tot;
    }
    if (threadIdx.x == 0 && (run + 1 != k || (k >= 2 && !top[0]))) atomicOr(&hdr[H_ERR], 128u);
}
__global__ void __launch_bounds__(NT) iota_kernel(uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i < n) out[i] = i;
}

struct InstArgs {
    uint32_t n;
    const uint32_t *top, *parent; // the kept topology; every index read from it is checked before it is used
    const uint2* child;
    uint32_t *counter, *hdr;
    float4 *leaf_box, *inner_box;
};
// boxes_kernel's climb and hand-off, inside the instance subtrees only: the lane pads its leaf's box with this pose's padding, then
// climbs while it is the second to reach a node and stops below the first top node (min / max are exact and rounding is monotone:
// the union of padded boxes is the padded union).  Nothing waits; a walk of more than n steps or an index out of range sets H_ERR.
__global__ void __launch_bounds__(NT) inst_boxes_kernel(InstArgs a)
{
    const uint32_t n = a.n;
    const uint32_t k = blockIdx.x * NT + threadIdx.x;
    if (k >= n) return;
    const float pad = frame_pad(a.hdr);
    float4 lo = a.leaf_box[2 * (size_t)k], hi = a.leaf_box[2 * (size_t)k + 1];
    lo.x -= pad; lo.y -= pad; lo.z -= pad;
    hi.x += pad; hi.y += pad; hi.z += pad;
    a.leaf_box[2 * (size_t)k] = lo;
    a.leaf_box[2 * (size_t)k + 1] = hi;
    if (n < 2) return;
    uint32_t p = a.parent[(size_t)(n - 1) + k];
    for (uint32_t steps = 0;; steps++) {
        if (p >= n - 1 || steps >= n) { atomicOr(&a.hdr[H_ERR], 256u); return; }
        if (a.top[p]) return; // the node below is an instance root
        const uint32_t before = __hip_atomic_fetch_add(&a.counter[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (before == 0) return; // the sibling's lane finishes this node
        const uint2 c = a.child[p];
        const uint32_t bx = (c.x & REF_LEAF) ? n : n - 1, by = (c.y & REF_LEAF) ? n : n - 1;
        if ((c.x & ~REF_LEAF) >= bx || (c.y & ~REF_LEAF) >= by) { atomicOr(&a.hdr[H_ERR], 256u); return; }
        float4 l0, h0, l1, h1;
        box_of(c.x, a.leaf_box, a.inner_box, l0, h0);
        box_of(c.y, a.leaf_box, a.inner_box, l1, h1);
        box_union(l0, h0, l1, h1);
        a.inner_box[2 * (size_t)p] = l0;
        a.inner_box[2 * (size_t)p + 1] = h0;
        if (p == 0) return;
        p = a.parent[p];
    }
}

// The top tree: agglomerative clustering of the k instance boxes in one workgroup (workgroup barriers only).  Per round every active
// cluster picks the partner of smallest union area (ties: the smaller slot); pairs that picked each other merge into the smaller
// slot, left child the smaller slot, and take their node ids in slot order.  The smallest pair of minimal area is always mutual, so
// a round merges at least one pair and k - 1 rounds suffice.  A box that encloses many others merges last and ends up under the root.
// Merge number m takes node top_ids[k - 2 - m]: the last one is the root, node 0.
struct TopArgs {
    uint32_t n, n_inst, k;
    const uint32_t *list, *root, *top, *top_ids;
    uint2 *child, *range;
    uint32_t* parent;
    const float4* leaf_box;
    float4* inner_box;
    uint32_t* hdr;
};
constexpr uint32_t TOP_NONE = 0xffffffffu;
using hjr::HJR_TOP_MAX;
// The clustering rounds of both top trees over k slots: box[0..2] the clusters' minima, box[3..5] their maxima, ref[s] == TOP_NONE: slot
// s is not an active cluster.  merge(s, j, idx) unites the mutual pair s < j, merge number idx in slot order, in slot s: it checks its
// bounds (false: one failed, nothing is written), calls cluster_union, names the new cluster in ref[s] and sets ref[j] = TOP_NONE.
// False: H_ERR bit 1024 is set and the workgroup returns.
__device__ __forceinline__ void cluster_union(float (&box)[6][HJR_TOP_MAX], uint32_t s, uint32_t j, float4& lo, float4& hi)
{
    float l[3], h[3];
    for (int ax = 0; ax < 3; ax++) {
        l[ax] = box[ax][s] = smin(box[ax][s], box[ax][j]);
        h[ax] = box[3 + ax][s] = smax(box[3 + ax][s], box[3 + ax][j]);
    }
    lo = make_float4(l[0], l[1], l[2], 0.0f);
    hi = make_float4(h[0], h[1], h[2], 0.0f);
}
template <class Merge>
__device__ __forceinline__ bool cluster_rounds(uint32_t k, float (&box)[6][HJR_TOP_MAX], const uint32_t* ref, uint32_t* partner, uint32_t* scan, uint32_t& err,
                                               uint32_t* hdr, Merge merge)
{
    uint32_t merged = 0;
    for (uint32_t round = 0; merged + 1 < k; round++) {
        if (round >= k) { if (threadIdx.x == 0) atomicOr(&hdr[H_ERR], 1024u); return false; } // (never: every round merges)
        for (uint32_t s = threadIdx.x; s < k; s += NT) {
            uint32_t bj = TOP_NONE;
            if (ref[s] != TOP_NONE) {
                const float lx = box[0][s], ly = box[1][s], lz = box[2][s], hx = box[3][s], hy = box[4][s], hz = box[5][s];
                float best = 0.0f;
                for (uint32_t j = 0; j < k; j++) {
                    if (j == s || ref[j] == TOP_NONE) continue;
                    const float dx = smax(hx, box[3][j]) - smin(lx, box[0][j]), dy = smax(hy, box[4][j]) - smin(ly, box[1][j]),
                                dz = smax(hz, box[5][j]) - smin(lz, box[2][j]);
                    const float area = dx * dy + dy * dz + dz * dx;
                    if (bj == TOP_NONE || area < best) { best = area; bj = j; }
                }
            }
            partner[s] = bj;
        }
        __syncthreads();
        // a thread owns four consecutive slots, so that the scan numbers the round's merges in slot order
        uint32_t mine = 0, tot;
        bool m[4];
        for (uint32_t q = 0; q < 4; q++) {
            const uint32_t s = 4 * threadIdx.x + q;
            const uint32_t j = s < k ? partner[s] : TOP_NONE;
            m[q] = j != TOP_NONE && j > s && j < k && partner[j] == s;
            mine += m[q] ? 1u : 0u;
        }
        uint32_t at = merged + block_scan(mine, tot, scan);
        for (uint32_t q = 0; q < 4; q++) {
            if (!m[q]) continue;
            const uint32_t s = 4 * threadIdx.x + q;
            if (!merge(s, partner[s], at++)) err = 1u;
        }
        __syncthreads();
        if (err || tot == 0) { if (threadIdx.x == 0) atomicOr(&hdr[H_ERR], 1024u); return false; } // (tot 0: a non-finite box, reported before this bit)
        merged += tot;
    }
    return true;
}
__global__ void __launch_bounds__(NT) inst_top_kernel(TopArgs a)
{
    __shared__ float s_box[6][HJR_TOP_MAX];
    __shared__ uint32_t s_ref[HJR_TOP_MAX], s_cnt[HJR_TOP_MAX], s_partner[HJR_TOP_MAX]; // s_ref: the cluster's BVH2 ref | s_cnt: its triangles
    __shared__ uint32_t s_scan[4], s_err;
    const uint32_t k = min(a.k, HJR_TOP_MAX), n = a.n;
    if (threadIdx.x == 0) s_err = 0u;
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < k; s += NT) {
        const uint32_t in = a.list[s];
        const uint32_t ref = in < a.n_inst ? a.root[in] : TOP_NONE;
        const uint32_t id = ref & ~REF_LEAF;
        const bool ok = ref != TOP_NONE && ((ref & REF_LEAF) ? id < n : (id + 1 < n && !a.top[id]));
        float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
        uint32_t cnt = 1;
        if (ok) {
            box_of(ref, a.leaf_box, a.inner_box, lo, hi);
            if (!(ref & REF_LEAF)) cnt = a.range[id].y;
        }
        if (!ok || cnt == 0) s_err = 1u;
        s_box[0][s] = lo.x; s_box[1][s] = lo.y; s_box[2][s] = lo.z;
        s_box[3][s] = hi.x; s_box[4][s] = hi.y; s_box[5][s] = hi.z;
        s_ref[s] = ref; s_cnt[s] = cnt;
    }
    __syncthreads();
    if (s_err) { if (threadIdx.x == 0) atomicOr(&a.hdr[H_ERR], 512u); return; }
    cluster_rounds(k, s_box, s_ref, s_partner, s_scan, s_err, a.hdr, [&](uint32_t s, uint32_t j, uint32_t idx) {
        const uint32_t id = idx + 2 <= k ? a.top_ids[k - 2 - idx] : TOP_NONE;
        const uint32_t rs = s_ref[s], rj = s_ref[j];
        const size_t ps = parent_slot((int)n, rs), pj = parent_slot((int)n, rj), slots = 2 * (size_t)n - 1;
        if (id + 1 >= n || id == TOP_NONE || !a.top[id] || ps >= slots || pj >= slots) return false;
        float4 lo, hi;
        cluster_union(s_box, s, j, lo, hi);
        s_cnt[s] += s_cnt[j];
        s_ref[s] = id;
        s_ref[j] = TOP_NONE;
        a.child[id] = make_uint2(rs, rj);
        a.range[id] = make_uint2(0u, s_cnt[s]); // only the count: a top node is never a BVH4 leaf
        a.inner_box[2 * (size_t)id] = lo;
        a.inner_box[2 * (size_t)id + 1] = hi;
        a.parent[ps] = id;
        a.parent[pj] = id;
        return true;
    });
}

// ---- grafted instance trees (option "device_bvh_graft") -----------------------------------------------------------------------------
// Skeleton, once per topology: the collapse's own kernels (wide_expand_kernel / wide_emit_kernel: emit_bvh4's rules on the object-space
// boxes) run level by level from a frontier that holds the root of every instance of more than leaf_max triangles, in instance order,
// so that ids are breadth-first over all instances together from 0.  Of the nodes they write only the refs rows are kept, with the
// parent slot of every node, and per instance the maxima of the pending-entry count and of the leaf depth below its root.
// Every commit: node_boxes_kernel (the refit's climb over the skeleton, into `stage` at the skeleton ids), graft_top_kernel (instance
// boxes, top tree, its collapse: the top nodes [0, base)), graft_place_kernel (stage -> nodes at base + id, base added to the inner
// refs).  The top-node count depends on the clustering, which needs this pose's instance boxes: it cannot be known before the boxes.
// H_ERR bits of these kernels: 8 / 16 skeleton refs, 32 skeleton parent, 64 a skeleton node that was not written, 512 instance roots,
// 1024 top tree, 2048 more nodes than the buffers hold.

// the frontier of the skeleton's first level and inst_ref of every non-empty instance (one workgroup; a thread owns four consecutive
// instances, so that the scan numbers the roots in instance order)
__global__ void __launch_bounds__(NT) skel_init_kernel(uint32_t n, uint32_t n_inst, uint32_t k, uint32_t leaf_max, const uint32_t* list, const uint32_t* root,
                                                       const uint32_t* top, const uint2* range, const uint32_t* pos, Front* fr, uint32_t* inst_ref, uint32_t* hdr)
{
    __shared__ uint32_t s_scan[4];
    uint32_t big[4], mine = 0, tot;
    bool bad = false;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        const uint32_t s = 4 * threadIdx.x + q;
        big[q] = SK_NONE;
        if (s >= k) continue;
        const uint32_t in = list[s];
        const uint32_t ref = in < n_inst ? root[in] : SK_NONE;
        const uint32_t id = ref & ~REF_LEAF;
        uint32_t leaf = HJR_LEAF_FLAG;
        if (ref == SK_NONE) bad = true;
        else if (ref & REF_LEAF) {
            if (id < n && pos[id] < n) leaf = HJR_LEAF_FLAG | (1u << 27) | pos[id];
            else bad = true;
        } else if (id + 1 < n && !top[id]) {
            const uint2 rg = range[id];
            if (rg.y == 0 || rg.x >= n || rg.y > n - rg.x) bad = true;
            else if (rg.y > leaf_max) { big[q] = id; mine++; }
            else leaf = HJR_LEAF_FLAG | (rg.y << 27) | rg.x;
        } else bad = true;
        inst_ref[s] = leaf;
    }
    uint32_t at = block_scan(mine, tot, s_scan);
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        if (big[q] == SK_NONE) continue;
        const uint32_t s = 4 * threadIdx.x + q;
        inst_ref[s] = at;
        fr[at++] = Front{ big[q], 0u, 0u, s };
    }
    if (bad) atomicOr(&hdr[H_ERR], 512u);
    if (threadIdx.x == 0) { hdr[H_BASE] = 0; hdr[H_F] = tot; }
}

// The top tree over the instance boxes and its BVH4, in one workgroup (workgroup barriers only).  An instance's box is the union of
// its root node's slot boxes in the stage, or of its triangles' padded boxes when it has no node.  Clustering: cluster_rounds
// (smallest union area, mutual pairs merge into the smaller slot, ties to the smaller slot); merge number m is binary node m, the
// last one the root.  Top-tree refs: an instance slot s < k, or k + m.  The binary tree is collapsed breadth-first with
// wide_expand_kernel's rule, where only binary nodes are expanded and an instance is a leaf slot (<= leaf_max triangles) or an inner
// slot (base + its root's skeleton id).  `base`, the number of top nodes, is what the first of two identical walks counts; the second
// one writes.  Boxes of instances and binary nodes live in a.box (global, written and read by this workgroup only, barriers between).
struct GraftTopArgs {
    uint32_t n, k, n_skel, cap;
    const uint32_t *inst_ref, *inst_stat;
    const float4 *stage, *geom;
    float4 *box, *nodes;
    uint32_t* hdr;
};
__device__ __forceinline__ uint32_t pick4(const uint32_t (&v)[4], uint32_t i) { return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3])); }
__device__ __forceinline__ void put4(uint32_t (&v)[4], uint32_t i, uint32_t x)
{
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) if (c == i) v[c] = x;
}
__global__ void __launch_bounds__(NT) graft_top_kernel(GraftTopArgs a)
{
    __shared__ float s_box[6][HJR_TOP_MAX];                       // the clusters' boxes; after the clustering the two frontiers
    __shared__ uint32_t s_ref[HJR_TOP_MAX], s_partner[HJR_TOP_MAX]; // s_ref TOP_NONE: the slot is not an active cluster
    __shared__ uint2 s_kid[HJR_TOP_MAX];                          // binary node m: its two top-tree refs
    __shared__ float s_area[HJR_TOP_MAX];                         // ... and its area (sah_area)
    __shared__ uint32_t s_scan[4], s_err;
    const uint32_t k = min(a.k, HJR_TOP_MAX), n = a.n;
    if (threadIdx.x == 0) s_err = 0u;
    __syncthreads();
    const float pad = frame_pad(a.hdr);
    for (uint32_t s = threadIdx.x; s < k; s += NT) {
        const uint32_t ref = a.inst_ref[s];
        float lo[3] = { EMPTY_LO, EMPTY_LO, EMPTY_LO }, hi[3] = { EMPTY_HI, EMPTY_HI, EMPTY_HI };
        if (ref_inner(ref)) {
            if (ref < a.n_skel) slots_box(a.stage + (size_t)ref * HJR_NODE4_F4, lo, hi);
            else s_err = 1u;
        } else {
            const uint32_t first = ref & 0x7ffffffu, cnt = (ref >> 27) & 15u;
            if (cnt > 0 && first < n && cnt <= n - first) rows_box(a.geom, first, cnt, pad, lo, hi);
            else s_err = 1u;
        }
        for (int ax = 0; ax < 3; ax++) { s_box[ax][s] = lo[ax]; s_box[3 + ax][s] = hi[ax]; }
        s_ref[s] = s;
        a.box[2 * (size_t)s] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        a.box[2 * (size_t)s + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
    __syncthreads();
    if (s_err) { if (threadIdx.x == 0) atomicOr(&a.hdr[H_ERR], 512u); return; }
    const bool clustered = cluster_rounds(k, s_box, s_ref, s_partner, s_scan, s_err, a.hdr, [&](uint32_t s, uint32_t j, uint32_t idx) {
        if (idx + 1 >= k) return false; // (never: k - 1 merges in all)
        float4 lo, hi;
        cluster_union(s_box, s, j, lo, hi);
        s_kid[idx] = make_uint2(s_ref[s], s_ref[j]);
        s_area[idx] = sah_area(lo, hi);
        s_ref[s] = k + idx;
        s_ref[j] = TOP_NONE;
        a.box[2 * (size_t)(k + idx)] = lo;
        a.box[2 * (size_t)(k + idx) + 1] = hi;
        return true;
    });
    if (!clustered) return;
    // the BVH4 of the top tree.  Frontier entries: top-tree ref, pending entries above the node, its binary depth
    uint32_t* fr = reinterpret_cast<uint32_t*>(&s_box[0][0]);
    uint32_t worst = 0, depth = 0, base = 0;
    const bool single_leaf = k == 1 && !ref_inner(a.inst_ref[0]); // one instance without a node: a root with one leaf slot
    for (int pass = (k == 1 && !single_leaf) ? 2 : 0; pass < 2; pass++) { // (one instance with nodes: its skeleton is the tree)
        uint32_t *cur = fr, *next = fr + 3 * HJR_TOP_MAX;
        uint32_t F = 1, lbase = 0;
        __syncthreads();
        if (threadIdx.x == 0) { cur[0] = k == 1 ? 0u : 2 * k - 2; cur[HJR_TOP_MAX] = 0u; cur[2 * HJR_TOP_MAX] = 0u; }
        __syncthreads();
        while (F > 0) {
            uint32_t run = 0;
            for (uint32_t chunk = 0; chunk < F; chunk += NT) {
                const uint32_t i = chunk + threadIdx.x;
                const bool valid = i < F;
                uint32_t ch[4] = { 0u, 0u, 0u, 0u }, dp[4] = { 0u, 0u, 0u, 0u }, nc = 0, ni = 0, pend = 0;
                if (valid) {
                    const uint32_t ref = cur[i], d0 = cur[2 * HJR_TOP_MAX + i];
                    pend = cur[HJR_TOP_MAX + i];
                    if (ref < k) { ch[0] = ref; dp[0] = d0; nc = 1; }
                    else {
                        const uint2 c = s_kid[ref - k];
                        ch[0] = c.x; ch[1] = c.y; dp[0] = dp[1] = d0 + 1; nc = 2;
                    }
                    while (nc < 4) { // replace the binary child of largest area by its two children
                        uint32_t best = 4;
                        float barea = -1.0f;
#pragma unroll
                        for (uint32_t c = 0; c < 4; c++)
                            if (c < nc && ch[c] >= k) { const float ar = s_area[ch[c] - k]; if (ar > barea) { barea = ar; best = c; } }
                        if (best == 4) break;
                        const uint2 c = s_kid[pick4(ch, best) - k];
                        const uint32_t dd = pick4(dp, best) + 1;
                        put4(ch, best, c.x); put4(dp, best, dd);
                        put4(ch, nc, c.y); put4(dp, nc, dd);
                        nc++;
                    }
#pragma unroll
                    for (uint32_t c = 0; c < 4; c++) ni += c < nc && ch[c] >= k ? 1u : 0u;
                }
                uint32_t tot;
                const uint32_t off = run + block_scan(ni, tot, s_scan);
                if (valid) {
                    const uint32_t h = pend + nc - 1;
                    worst = max(worst, h);
                    float q[28];
                    uint32_t k_in = 0;
#pragma unroll
                    for (uint32_t c = 0; c < 4; c++) {
                        uint32_t ref = HJR_LEAF_FLAG;
                        float4 lo = make_float4(EMPTY_LO, EMPTY_LO, EMPTY_LO, 0.0f), hi = make_float4(EMPTY_HI, EMPTY_HI, EMPTY_HI, 0.0f);
                        if (c < nc) {
                            const uint32_t r = ch[c];
                            if (r >= k) {
                                const uint32_t j = off + k_in++;
                                ref = lbase + F + j;
                                if (j < HJR_TOP_MAX) { next[j] = r; next[HJR_TOP_MAX + j] = h; next[2 * HJR_TOP_MAX + j] = dp[c]; }
                            } else {
                                const uint32_t ir = a.inst_ref[r];
                                if (ref_inner(ir)) {
                                    ref = base + ir;
                                    worst = max(worst, h + a.inst_stat[2 * (size_t)r]);
                                    depth = max(depth, dp[c] + a.inst_stat[2 * (size_t)r + 1]);
                                } else {
                                    ref = ir;
                                    depth = max(depth, dp[c]);
                                }
                            }
                            if (pass == 1) { lo = a.box[2 * (size_t)r]; hi = a.box[2 * (size_t)r + 1]; }
                        }
                        q[c] = lo.x; q[4 + c] = hi.x; q[8 + c] = lo.y; q[12 + c] = hi.y; q[16 + c] = lo.z; q[20 + c] = hi.z;
                        q[24 + c] = __uint_as_float(ref);
                    }
                    if (pass == 1 && lbase + i < a.cap) store_node(a.nodes + (size_t)(lbase + i) * HJR_NODE4_F4, q);
                }
                run += tot;
            }
            __syncthreads();
            lbase += F;
            F = min(run, HJR_TOP_MAX);
            uint32_t* t = cur; cur = next; next = t;
        }
        if (pass == 0) { base = lbase; worst = 0; depth = 0; }
    }
    if (k == 1 && !single_leaf && threadIdx.x == 0) { worst = a.inst_stat[0]; depth = a.inst_stat[1]; }
    if (worst) atomicMax(&a.hdr[H_WORST], worst);
    if (depth) atomicMax(&a.hdr[H_DEPTH], depth);
    if (threadIdx.x == 0) {
        if (base > a.cap || a.n_skel > a.cap - base) atomicOr(&a.hdr[H_ERR], 2048u);
        else { a.hdr[H_F] = base; a.hdr[H_BASE] = base + a.n_skel; } // the top-node count for graft_place_kernel, all nodes for the cost
    }
}

// stage -> nodes behind the hdr[H_F] top nodes, one lane per float4; the inner refs of a refs row become final ids
__global__ void __launch_bounds__(NT) graft_place_kernel(uint32_t n_skel, uint32_t cap, const float4* stage, const uint32_t* counter, float4* nodes, uint32_t* hdr)
{
    const size_t t = (size_t)blockIdx.x * NT + threadIdx.x;
    if (t >= (size_t)n_skel * HJR_NODE4_F4) return;
    const uint32_t base = hdr[H_F], id = (uint32_t)(t / HJR_NODE4_F4);
    if (base > cap || n_skel > cap - base) return; // (graft_top_kernel set the bit)
    float4 x = stage[t];
    if (t % HJR_NODE4_F4 == 6) {
        if (counter[id] != inner_slots(x)) atomicOr(&hdr[H_ERR], 64u); // its children did not all arrive: the node was never written
        uint32_t r[4] = { __float_as_uint(x.x), __float_as_uint(x.y), __float_as_uint(x.z), __float_as_uint(x.w) };
#pragma unroll
        for (int c = 0; c < 4; c++) if (ref_inner(r[c])) r[c] += base;
        x = make_float4(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[3]));
    }
    nodes[(size_t)base * HJR_NODE4_F4 + t] = x;
}

inline unsigned blocks_for(size_t n) { return (unsigned)std::max<size_t>(1, (n + NT - 1) / NT); }

} // namespace

namespace hjr {

void DeviceBvh::release()
{
    have_scene = false;
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    ev0 = ev1 = nullptr;
}

#define DCHK(call)                                                                                           \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) { err = std::string(#call) + " failed: " + hipGetErrorString(e_); return HJR_ERR_DEVICE; } \
    } while (0)

static int fail_alloc(std::string& err)
{
    err = "device BVH: allocation or upload failed";
    return HJR_ERR_DEVICE;
}

// the object-space scene, once per hjr_upload_scene; a topology of the scene before it is no longer valid
static bool upload_scene(DeviceBvh& b, const SceneCopy& sc, hipStream_t st)
{
    if (b.have_scene) return true;
    if (!b.vert.upload(sc.vertices.data(), sc.vertices.size() * 4, st) || !b.norm.upload(sc.normals.data(), sc.normals.size() * 4, st) ||
        !b.uv.upload(sc.texcoords.data(), sc.texcoords.size() * 4, st) || !b.idx.upload(sc.indices.data(), sc.indices.size() * 4, st) ||
        !b.mat.upload(sc.material_ids.data(), sc.material_ids.size() * 4, st) || !b.prim_off.upload(sc.prim_offset.data(), sc.prim_offset.size() * 4, st))
        return false;
    b.have_scene = true;
    b.topo.valid = false;
    return true;
}

static bool morph_active(const DeviceMorph* dm) { return dm && dm->host && dm->host->active() && dm->w_next; }

// The working arrays of a morphed scene for this commit's weights, on `st` ahead of the flatten; the object-space scene is on the device.
// Once per hjr_set_morph: deltas and set table.  Once per change of the base: a device copy of the base arrays.  Per commit: the weights
// and one hjr_morph_kernel over the sets' vertices, unless the working arrays already hold this blend.
static int prepare_morph(DeviceBvh& b, const SceneCopy& sc, DeviceMorph* dm, hipStream_t st, std::string& err)
{
    if (!morph_active(dm)) return HJR_OK;
    const Morph& mo = *dm->host;
    const size_t base_bytes = sc.vertices.size() * 4, nw = mo.weights.size();
    std::vector<MorphSetDev> table;
    uint32_t blocks = 0;
    for (const MorphSet& s : mo.sets) {
        table.push_back({ s.first_vertex, s.n_vertices, s.n_targets, s.first_weight, blocks, s.nrm != Morph::NONE ? 1u : 0u, (unsigned long long)s.pos,
                          s.nrm != Morph::NONE ? (unsigned long long)s.nrm : 0ull });
        blocks += (s.n_vertices + NT - 1) / NT;
    }
    if (!dm->uploaded) {
        if (!dm->deltas.upload(mo.deltas.data(), mo.deltas.size() * 4, st) || !dm->table.upload(table.data(), table.size() * sizeof(MorphSetDev), st) ||
            !dm->vert.reserve(base_bytes) || !dm->norm.reserve(base_bytes) || !dm->weights.reserve(std::max<size_t>(nw, 1) * 4))
            return fail_alloc(err);
        DCHK(hipStreamSynchronize(st)); // `table` is a local
        dm->uploaded = true;
        dm->copied = false;
    }
    if (!dm->copied) {
        DCHK(hipMemcpyAsync(dm->vert.p, b.vert.p, base_bytes, hipMemcpyDeviceToDevice, st));
        DCHK(hipMemcpyAsync(dm->norm.p, b.norm.p, base_bytes, hipMemcpyDeviceToDevice, st));
        dm->copied = true;
        dm->blended = false;
    }
    if (dm->blended && dm->w.size() == nw && memcmp(dm->w.data(), dm->w_next, nw * 4) == 0) return HJR_OK;
    dm->w.assign(dm->w_next, dm->w_next + nw); // kept: the source of the copy below
    DCHK(hipMemcpyAsync(dm->weights.p, dm->w.data(), nw * 4, hipMemcpyHostToDevice, st));
    MorphArgs a = { b.vert.as<float>(), b.norm.as<float>(), dm->deltas.as<float>(), dm->weights.as<float>(), dm->table.as<MorphSetDev>(), (uint32_t)table.size(),
                    dm->vert.as<float>(), dm->norm.as<float>() };
    if (!dm->ev0) DCHK(hipEventCreate(&dm->ev0));
    if (!dm->ev1) DCHK(hipEventCreate(&dm->ev1));
    DCHK(hipEventRecord(dm->ev0, st));
    hipLaunchKernelGGL(hjr_morph_kernel, dim3(blocks), dim3(NT), 0, st, a);
    DCHK(hipEventRecord(dm->ev1, st));
    DCHK(hipGetLastError());
    dm->blended = true;
    dm->launched += mo.n_vertices;
    return HJR_OK;
}

// what b.xf takes per instance: 12 floats of M, then 12 of Mi (the caller keeps it until its host wait)
static std::vector<float> pack_transforms(const float* M, const float* Mi, uint32_t n_inst)
{
    std::vector<float> xf((size_t)n_inst * 24);
    for (uint32_t i = 0; i < n_inst; i++) {
        memcpy(&xf[24 * (size_t)i], M + 12 * (size_t)i, 48);
        memcpy(&xf[24 * (size_t)i + 12], Mi + 12 * (size_t)i, 48);
    }
    return xf;
}

// the scene (under a morph: its working arrays), the transforms and the builder's per-triangle buffers; a kernel reads only those its pass has reserved
static FlattenArgs flatten_args(const DeviceBvh& b, const DeviceMorph* dm, uint32_t n, uint32_t n_inst)
{
    FlattenArgs fa;
    const bool morphed = morph_active(dm); // the working arrays prepare_morph made current
    fa.vert = (morphed ? dm->vert : b.vert).as<float>(); fa.norm = (morphed ? dm->norm : b.norm).as<float>(); fa.uv = b.uv.as<float>(); fa.xf = b.xf.as<float>();
    fa.idx = b.idx.as<uint32_t>(); fa.mat = b.mat.as<uint32_t>(); fa.prim_off = b.prim_off.as<uint32_t>();
    fa.n = n; fa.n_inst = n_inst;
    fa.wv = b.wv.as<float>(); fa.shade = b.tri_shade.as<float>(); fa.box = b.box.as<float>(); fa.cent = b.cent.as<float>();
    fa.inst = b.tri_inst.as<uint32_t>(); fa.hdr = b.hdr.as<uint32_t>();
    return fa;
}

static int scan(uint32_t* in_out, const uint32_t* n_ptr, uint32_t n_const, uint32_t* part, uint32_t* total, hipStream_t st, std::string& err)
{
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(SCAN_G), dim3(NT), 0, st, in_out, n_ptr, n_const, part);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(NT), 0, st, part, total);
    hipLaunchKernelGGL(scan_down_kernel, dim3(SCAN_G), dim3(NT), 0, st, in_out, in_out, n_ptr, n_const, part);
    DCHK(hipGetLastError());
    return HJR_OK;
}

// the tree cost of `nodes` (their count at *n_ptr, at most cap) into hdr[H_SAH]
static void launch_sah(DeviceBvh& b, const float4* nodes, const uint32_t* n_ptr, uint32_t cap, const uint32_t* counter, hipStream_t st)
{
    uint32_t* hdr = b.hdr.as<uint32_t>();
    hipLaunchKernelGGL(sah_reduce_kernel, dim3(SCAN_G), dim3(NT), 0, st, nodes, n_ptr, cap, counter, b.part.as<float>(), hdr);
    hipLaunchKernelGGL(sah_top_kernel, dim3(1), dim3(NT), 0, st, nodes, b.part.as<const float>(), hdr);
}

// stable sort of keys[0] / vals[0] (n pairs, nb tiles): 8 x 8 bits, the result is back in keys[0] / vals[0]
static int sort_pairs(DeviceBvh& b, uint32_t n, uint32_t nb, hipStream_t st, std::string& err)
{
    uint64_t* keys[2] = { b.keys[0].as<uint64_t>(), b.keys[1].as<uint64_t>() };
    uint32_t* vals[2] = { b.vals[0].as<uint32_t>(), b.vals[1].as<uint32_t>() };
    for (int pass = 0; pass < 8; pass++) {
        const int s = pass & 1;
        hipLaunchKernelGGL(radix_hist_kernel, dim3(nb), dim3(NT), 0, st, keys[s], n, 8 * pass, b.hist.as<uint32_t>(), nb);
        if (const int rc = scan(b.hist.as<uint32_t>(), nullptr, nb * 256u, b.part.as<uint32_t>(), nullptr, st, err)) return rc;
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(nb), dim3(NT), 0, st, keys[s], vals[s], n, 8 * pass, b.hist.as<uint32_t>(), nb, keys[s ^ 1], vals[s ^ 1]);
    }
    return HJR_OK;
}

// The boxes of the BVH2 (child, parent) over n >= 2 sorted leaves into b.inner_box, bottom-up from b.leaf_box; with `order`, the leaf
// boxes are first gathered from b.box in that order.
static int bvh2_boxes(DeviceBvh& b, uint32_t n, const uint32_t* order, const uint2* child, const uint32_t* parent, hipStream_t st, std::string& err)
{
    if (order)
        hipLaunchKernelGGL(gather_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, n, order, nullptr, nullptr, b.mat.as<uint32_t>(), b.box.as<float>(), nullptr,
                           b.leaf_box.as<float>());
    DCHK(hipMemsetAsync(b.counter.p, 0, (size_t)(n - 1) * 4, st));
    hipLaunchKernelGGL(boxes_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, (int)n, child, parent, b.counter.as<uint32_t>(), b.leaf_box.as<float4>(),
                       b.inner_box.as<float4>());
    return HJR_OK;
}

// Option "device_bvh_opt": the treelet rounds over the BVH2 (child, parent; its boxes in b.leaf_box / b.inner_box; `top` as TreeletArgs),
// then every sorted leaf's tri_geom row into `pos` and the inner nodes' (first, count) into `range`.
static int restructure_bvh2(DeviceBvh& b, uint32_t n, uint32_t leaf_max, uint32_t opt_rounds, uint2* child, uint32_t* parent, const uint32_t* top, uint32_t* pos,
                            uint2* range, hipStream_t st, std::string& err)
{
    TreeletArgs ta;
    ta.n = (int)n; ta.leaf_max = leaf_max;
    ta.child = child; ta.parent = parent; ta.counter = b.counter.as<uint32_t>();
    ta.count = b.node_count.as<uint32_t>(); ta.cost = b.node_cost.as<float>();
    ta.leaf_box = b.leaf_box.as<float4>(); ta.inner_box = b.inner_box.as<float4>(); ta.top = top;
    for (uint32_t round = 0; round < opt_rounds; round++) {
        ta.gamma = TREELET << round; // the paper's schedule: the treelet size, doubled every round
        DCHK(hipMemsetAsync(b.counter.p, 0, (size_t)(n - 1) * 4, st));
        hipLaunchKernelGGL(treelet_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, ta);
    }
    hipLaunchKernelGGL(leaf_pos_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, (int)n, child, parent, ta.count, pos, b.hdr.as<uint32_t>());
    hipLaunchKernelGGL(inner_range_kernel, dim3(blocks_for(n - 1)), dim3(NT), 0, st, (int)n, child, ta.count, pos, range, b.hdr.as<uint32_t>());
    return HJR_OK;
}

// The collapse's levels -> b.nodes, from the frontier in b.frontier[0] with hdr[H_BASE] / hdr[H_F] set: LEVEL_BATCH levels between two
// reads of the frontier size.  F: the nodes still to expand when the levels ran out (0: the tree is complete, its size in hdr[H_BASE]).
static int collapse_levels(DeviceBvh& b, const CollapseArgs& ca, size_t nn, hipStream_t st, uint32_t& F, std::string& err)
{
    uint32_t* hdr = ca.hdr;
    Front* fr[2] = { b.frontier[0].as<Front>(), b.frontier[1].as<Front>() };
    Wide* wide = b.wide.as<Wide>();
    uint32_t* n_inner = reinterpret_cast<uint32_t*>(b.wide.as<char>() + nn * sizeof(Wide));
    const unsigned grid = (unsigned)std::min<size_t>(blocks_for(nn), 1024);
    uint32_t level = 0;
    F = 1;
    while (F > 0 && level < hjr::DEVICE_BVH_MAX_STACK) {
        for (int k = 0; k < LEVEL_BATCH; k++, level++) {
            hipLaunchKernelGGL(wide_expand_kernel, dim3(grid), dim3(NT), 0, st, ca, fr[level & 1], wide, n_inner);
            if (const int rc = scan(n_inner, hdr + H_F, 0u, b.part.as<uint32_t>(), hdr + H_NEXT, st, err)) return rc;
            hipLaunchKernelGGL(wide_emit_kernel, dim3(grid), dim3(NT), 0, st, ca, wide, n_inner, fr[(level + 1) & 1], b.nodes.as<float4>());
            hipLaunchKernelGGL(level_advance_kernel, dim3(1), dim3(1), 0, st, hdr);
        }
        DCHK(hipGetLastError());
        DCHK(hipMemcpyAsync(&F, hdr + H_F, 4, hipMemcpyDeviceToHost, st));
        DCHK(hipStreamSynchronize(st));
    }
    return HJR_OK;
}

// The one read of the header that ends a build, a refit or a commit: the host wait, the HIP-event time since ev0, the checks and the
// results.  `what` names the tree in the structural-bound error.
static int read_header(DeviceBvh& b, hipStream_t st, DeviceBvhResult& r, const char* what, std::string& err)
{
    DCHK(hipEventRecord(b.ev1, st));
    uint32_t h[H_WORDS];
    DCHK(hipMemcpyAsync(h, b.hdr.p, sizeof(h), hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    DCHK(hipEventElapsedTime(&r.build_ms, b.ev0, b.ev1));
    const float smax_v = __builtin_bit_cast(float, h[H_SMAX]);
    if (!(smax_v < 1e30f)) { err = "non-finite vertex after transform"; return HJR_ERR_ARG; }
    if (h[H_ERR]) { err = std::string(what) + " failed a structural bound (" + std::to_string(h[H_ERR]) + ")"; return HJR_ERR_DEVICE; }
    r.n_nodes = h[H_BASE];
    r.sah = __builtin_bit_cast(float, h[H_SAH]);
    r.stack_need = std::max<uint32_t>(h[H_WORST], 1u) + 1;
    r.depth = h[H_DEPTH];
    return HJR_OK;
}

// The BVH2 `ca` describes over n >= 1 triangles -> b.nodes, level by level; then the tree cost, the build's one read of the header
// and its results.
static int collapse_and_cost(DeviceBvh& b, const CollapseArgs& ca, uint32_t n, size_t nn, hipStream_t st, DeviceBvhResult& r, const char* what, std::string& err)
{
    hipLaunchKernelGGL(collapse_init_kernel, dim3(1), dim3(1), 0, st, n, b.frontier[0].as<Front>(), ca.hdr);
    uint32_t F;
    if (const int rc = collapse_levels(b, ca, nn, st, F, err)) return rc;
    launch_sah(b, b.nodes.as<float4>(), ca.hdr + H_BASE, (uint32_t)nn, nullptr, st);
    DCHK(hipGetLastError());
    if (const int rc = read_header(b, st, r, what, err)) return rc;
    if (F > 0 || r.stack_need > hjr::DEVICE_BVH_MAX_STACK) { err = "BVH deeper than the traversal stack"; r.too_deep = true; return HJR_ERR_ARG; }
    return HJR_OK;
}

int device_bvh_build(DeviceBvh& b, const SceneCopy& sc, const float* M, const float* Mi, uint32_t n_inst, uint32_t leaf_max, uint32_t opt_rounds,
                     const float* lights, size_t light_floats, hipStream_t st, DeviceBvhResult& r, std::string& err, DeviceMorph* dm)
{
    const uint32_t n = sc.n_triangles;
    r = DeviceBvhResult();
    if (!b.ev0) DCHK(hipEventCreate(&b.ev0));
    if (!b.ev1) DCHK(hipEventCreate(&b.ev1));
    if (!upload_scene(b, sc, st)) return fail_alloc(err);
    if (const int rc = prepare_morph(b, sc, dm, st, err)) return rc;
    const std::vector<float> xf = pack_transforms(M, Mi, n_inst);
    const size_t nn = std::max<uint32_t>(n, 1u);            // node / frontier capacity: a wide node takes at least one BVH2 inner node
    const uint32_t nb = (uint32_t)((n + SORT_TILE - 1) / SORT_TILE);
    if (!b.xf.upload(xf.data(), xf.size() * 4, st) || !b.lights.upload(lights, light_floats * 4, st) || !b.hdr.reserve(H_WORDS * 4) ||
        !b.nodes.reserve(nn * HJR_NODE4_F4 * 16) || !b.tri_geom.reserve(nn * HJR_TRI_F4 * 16) || !b.tri_shade.reserve(nn * HJR_SHADE_F4 * 16) ||
        !b.tri_inst.reserve(nn * 4) || !b.wv.reserve(nn * 36) || !b.box.reserve(nn * 32) || !b.cent.reserve(nn * 16) || !b.keys[0].reserve(nn * 8) ||
        !b.keys[1].reserve(nn * 8) || !b.vals[0].reserve(nn * 4) || !b.vals[1].reserve(nn * 4) || !b.hist.reserve(std::max<size_t>(1, (size_t)nb * 256 * 4)) ||
        !b.part.reserve(SCAN_G * 4) || !b.leaf_box.reserve(nn * 32) || !b.inner_box.reserve(nn * 32) || !b.inner_child.reserve(nn * 8) ||
        !b.inner_range.reserve(nn * 8) || !b.parent.reserve(2 * nn * 4) || !b.counter.reserve(nn * 4) || !b.frontier[0].reserve(nn * sizeof(Front)) ||
        !b.frontier[1].reserve(nn * sizeof(Front)) || !b.wide.reserve(nn * (sizeof(Wide) + 4)))
        return fail_alloc(err);
    const bool restructure = opt_rounds > 0 && n >= 2;
    if (restructure && (!b.node_count.reserve(nn * 4) || !b.node_cost.reserve(nn * 4) || !b.leaf_pos.reserve(nn * 4)))
        return fail_alloc(err);
    uint32_t* hdr = b.hdr.as<uint32_t>();
    DCHK(hipEventRecord(b.ev0, st));
    hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(64), 0, st, hdr);
    if (n == 0) { // empty scene: one root with four empty slots (frame.cpp:614-624), one zero triangle record
        float q[28];
        for (int c = 0; c < 4; c++) empty_slot(q, c);
        DCHK(hipMemcpyAsync(b.nodes.p, q, sizeof(q), hipMemcpyHostToDevice, st));
        DCHK(hipMemsetAsync(b.tri_geom.p, 0, HJR_TRI_F4 * 16, st));
        DCHK(hipEventRecord(b.ev1, st));
        DCHK(hipStreamSynchronize(st));
        r.n_nodes = 1; r.stack_need = 2; r.depth = 0;
        DCHK(hipEventElapsedTime(&r.build_ms, b.ev0, b.ev1));
        return HJR_OK;
    }
    uint2* child = b.inner_child.as<uint2>();
    uint32_t *parent = b.parent.as<uint32_t>(), *order = b.vals[0].as<uint32_t>();
    hipLaunchKernelGGL(flatten_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, flatten_args(b, dm, n, n_inst));
    hipLaunchKernelGGL(morton_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, n, b.box.as<float>(), b.cent.as<float>(), hdr, b.keys[0].as<uint64_t>(), order);
    if (const int rc = sort_pairs(b, n, nb, st, err)) return rc;
    // with a restructuring, tri_geom waits for the leaves' new positions
    hipLaunchKernelGGL(gather_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, n, order, nullptr, b.wv.as<float>(), b.mat.as<uint32_t>(), b.box.as<float>(),
                       restructure ? nullptr : b.tri_geom.as<float>(), b.leaf_box.as<float>());
    if (n >= 2) {
        hipLaunchKernelGGL(karras_kernel, dim3(blocks_for(n - 1)), dim3(NT), 0, st, (int)n, b.keys[0].as<uint64_t>(), child, b.inner_range.as<uint2>(), parent);
        if (const int rc = bvh2_boxes(b, n, nullptr, child, parent, st, err)) return rc;
    }
    if (restructure) { // option "device_bvh_opt"
        if (const int rc = restructure_bvh2(b, n, leaf_max, opt_rounds, child, parent, nullptr, b.leaf_pos.as<uint32_t>(), b.inner_range.as<uint2>(), st, err)) return rc;
        hipLaunchKernelGGL(gather_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, n, order, b.leaf_pos.as<uint32_t>(), b.wv.as<float>(), b.mat.as<uint32_t>(),
                           b.box.as<float>(), b.tri_geom.as<float>(), nullptr);
    }
    DCHK(hipGetLastError());
    CollapseArgs ca;
    ca.child = child; ca.range = b.inner_range.as<uint2>();
    ca.leaf_box = b.leaf_box.as<float4>(); ca.inner_box = b.inner_box.as<float4>();
    ca.leaf_pos = restructure ? b.leaf_pos.as<uint32_t>() : nullptr;
    ca.leaf_max = leaf_max; ca.cap = (uint32_t)nn; ca.hdr = hdr;
    ca.top = nullptr; ca.inst_stat = nullptr;
    return collapse_and_cost(b, ca, n, nn, st, r, "device BVH: the restructured tree", err);
}

int device_bvh_refit(DeviceBvh& b, const SceneCopy& sc, const float* M, const float* Mi, uint32_t n_inst, const DevBuf& cur_nodes, const DevBuf& cur_geom,
                     uint32_t n_nodes, const float* lights, size_t light_floats, hipStream_t st, DeviceBvhResult& r, std::string& err, DeviceMorph* dm)
{
    const uint32_t n = sc.n_triangles;
    r = DeviceBvhResult();
    const size_t node_bytes = (size_t)n_nodes * HJR_NODE4_F4 * 16, geom_bytes = (size_t)n * HJR_TRI_F4 * 16;
    if (!b.have_scene || !b.ev0 || !b.ev1 || n < 2 || n_nodes == 0 || n_nodes > n || cur_nodes.cap < node_bytes || cur_geom.cap < geom_bytes) {
        err = "device BVH refit: no device-built frame data of this scene";
        return HJR_ERR_DEVICE;
    }
    if (const int rc = prepare_morph(b, sc, dm, st, err)) return rc;
    const std::vector<float> xf = pack_transforms(M, Mi, n_inst);
    if (!b.xf.upload(xf.data(), xf.size() * 4, st) || !b.lights.upload(lights, light_floats * 4, st) || !b.hdr.reserve(H_WORDS * 4) || !b.nodes.reserve(node_bytes) ||
        !b.tri_geom.reserve(geom_bytes) || !b.tri_shade.reserve((size_t)n * HJR_SHADE_F4 * 16) || !b.tri_inst.reserve((size_t)n * 4) ||
        !b.parent.reserve((size_t)n_nodes * 4) || !b.counter.reserve((size_t)n_nodes * 4) || !b.part.reserve(SCAN_G * 4))
        return fail_alloc(err);
    uint32_t* hdr = b.hdr.as<uint32_t>();
    const float4* refs = cur_nodes.as<float4>() + 6; // only the refs rows and the prim ids of the current frame data are read
    LeafFlattenArgs fa = { flatten_args(b, dm, n, n_inst), cur_geom.as<float4>(), nullptr, nullptr, b.tri_geom.as<float4>(), nullptr };
    NodeBoxArgs na = { n, n_nodes, refs, HJR_NODE4_F4, false, b.tri_geom.as<float4>(), b.nodes.as<float4>(), b.parent.as<uint32_t>(), b.counter.as<uint32_t>(), hdr };
    DCHK(hipEventRecord(b.ev0, st));
    hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(64), 0, st, hdr);
    DCHK(hipMemsetAsync(b.parent.p, 0xff, (size_t)n_nodes * 4, st)); // a node no slot refers to has no parent below it
    DCHK(hipMemsetAsync(b.counter.p, 0, (size_t)n_nodes * 4, st));
    hipLaunchKernelGGL(leaf_flatten_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, fa);
    hipLaunchKernelGGL(node_parent_kernel, dim3(blocks_for(n_nodes)), dim3(NT), 0, st, n_nodes, refs, (uint32_t)HJR_NODE4_F4, n, nullptr, b.parent.as<uint32_t>(), hdr);
    hipLaunchKernelGGL(node_boxes_kernel, dim3(blocks_for(n_nodes)), dim3(NT), 0, st, na);
    hipLaunchKernelGGL(set_word_kernel, dim3(1), dim3(1), 0, st, hdr + H_BASE, n_nodes);
    launch_sah(b, b.nodes.as<float4>(), hdr + H_BASE, n_nodes, b.counter.as<uint32_t>(), st);
    DCHK(hipGetLastError());
    if (const int rc = read_header(b, st, r, "device BVH refit: the current tree", err)) return rc; // the refit's one host wait
    r.stack_need = r.depth = 0; // the topology's, which the caller has
    return HJR_OK;
}

// The skeleton of option "device_bvh_graft" (kernel comment above) from the finished BVH2 of b.topo: the collapse's level loop from the
// instance roots, into b.nodes as scratch; then the BVH2 is freed.  b.leaf_box / b.inner_box hold the object-space boxes.
static int build_skeleton(DeviceBvh& b, uint32_t n, uint32_t n_inst, uint32_t leaf_max, bool have_boxes, hipStream_t st, std::string& err)
{
    DeviceBvh::Topology& T = b.topo;
    const size_t nn = std::max<uint32_t>(n, 1u);
    const uint32_t k = T.k;
    uint32_t* hdr = b.hdr.as<uint32_t>();
    if (!T.inst_ref.reserve((size_t)k * 4) || !T.inst_stat.reserve((size_t)k * 8) || !T.top_box.reserve((size_t)k * 64)) return fail_alloc(err);
    if (!have_boxes && n >= 2) // without treelet rounds the topology build had no use for the object-space node boxes
        if (const int rc = bvh2_boxes(b, n, T.order.as<uint32_t>(), T.child.as<uint2>(), T.parent.as<uint32_t>(), st, err)) return rc;
    DCHK(hipMemsetAsync(T.inst_stat.p, 0, (size_t)k * 8, st));
    hipLaunchKernelGGL(skel_init_kernel, dim3(1), dim3(NT), 0, st, n, n_inst, k, leaf_max, T.list.as<uint32_t>(), T.root.as<uint32_t>(), T.top.as<uint32_t>(),
                       T.range.as<uint2>(), T.pos.as<uint32_t>(), b.frontier[0].as<Front>(), T.inst_ref.as<uint32_t>(), hdr);
    CollapseArgs ca;
    ca.child = T.child.as<uint2>(); ca.range = T.range.as<uint2>();
    ca.leaf_box = b.leaf_box.as<float4>(); ca.inner_box = b.inner_box.as<float4>();
    ca.leaf_pos = T.pos.as<uint32_t>();
    ca.leaf_max = leaf_max; ca.cap = (uint32_t)nn; ca.hdr = hdr;
    ca.top = nullptr; // nothing under an instance root is a top node
    ca.inst_stat = T.inst_stat.as<uint32_t>();
    uint32_t F, S = 0;
    if (const int rc = collapse_levels(b, ca, nn, st, F, err)) return rc;
    DCHK(hipMemcpyAsync(&S, hdr + H_BASE, 4, hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    T.skel_deep = F > 0;
    T.n_skel = S = std::min<uint32_t>(S, (uint32_t)nn);
    if (!T.skel_refs.reserve(std::max<size_t>(1, (size_t)S * 16)) || !T.skel_parent.reserve(std::max<size_t>(1, (size_t)S * 4)) ||
        !b.stage.reserve(std::max<size_t>(1, (size_t)S * HJR_NODE4_F4 * 16)))
        return fail_alloc(err);
    DCHK(hipMemsetAsync(T.skel_parent.p, 0xff, (size_t)S * 4, st));
    // what is kept of the S nodes the collapse wrote: the refs rows, and 4 * parent + slot of every node an inner slot refers to
    if (S) hipLaunchKernelGGL(node_parent_kernel, dim3(blocks_for(S)), dim3(NT), 0, st, S, b.nodes.as<float4>() + 6, (uint32_t)HJR_NODE4_F4, 0u, T.skel_refs.as<float4>(),
                              T.skel_parent.as<uint32_t>(), hdr);
    DCHK(hipGetLastError());
    return HJR_OK;
}

// The topology of option "device_bvh_instances" into b.topo (kernel comment above); the object-space scene is on the device and the
// build's scratch is reserved.  One host wait; b.topo.ms is its HIP-event time.
static int build_topology(DeviceBvh& b, const DeviceMorph* dm, uint32_t n, uint32_t n_inst, uint32_t leaf_max, uint32_t opt_rounds, bool graft,
                          const std::vector<uint32_t>& list, hipStream_t st, std::string& err)
{
    DeviceBvh::Topology& T = b.topo;
    T.valid = false;
    const size_t nn = std::max<uint32_t>(n, 1u);
    const uint32_t k = (uint32_t)list.size(), nb = (uint32_t)((n + SORT_TILE - 1) / SORT_TILE);
    if (!T.child.reserve(nn * 8) || !T.range.reserve(nn * 8) || !T.parent.reserve(2 * nn * 4) || !T.pos.reserve(nn * 4) || !T.order.reserve(nn * 4) ||
        !T.top.reserve(nn * 4) || !T.top_ids.reserve((size_t)std::max(k, 1u) * 4) || !T.root.reserve((size_t)std::max(n_inst, 1u) * 4) ||
        !T.bounds.reserve((size_t)std::max(n_inst, 1u) * 24) || !T.list.upload(list.data(), list.size() * 4, st))
        return fail_alloc(err);
    int bits = 0;
    while (bits < 32 && (1ull << bits) < n_inst) bits++;
    const int shift = 63 - bits;
    uint32_t* hdr = b.hdr.as<uint32_t>();
    uint32_t *bmin = T.bounds.as<uint32_t>(), *bmax = bmin + 3 * (size_t)n_inst;
    uint64_t* keys = b.keys[0].as<uint64_t>();
    uint32_t *vals = b.vals[0].as<uint32_t>(), *parent = T.parent.as<uint32_t>(), *top = T.top.as<uint32_t>();
    uint2 *child = T.child.as<uint2>(), *range = T.range.as<uint2>();
    const bool restructure = opt_rounds > 0 && n >= 2;
    DCHK(hipEventRecord(b.ev0, st));
    hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(64), 0, st, hdr);
    DCHK(hipMemsetAsync(bmin, 0xff, (size_t)n_inst * 12, st));
    DCHK(hipMemsetAsync(bmax, 0, (size_t)n_inst * 12, st));
    DCHK(hipMemsetAsync(T.root.p, 0xff, (size_t)n_inst * 4, st));
    hipLaunchKernelGGL(obj_box_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, flatten_args(b, dm, n, n_inst), bmin, bmax); // tri_inst: scratch until the commit's flatten
    hipLaunchKernelGGL(obj_morton_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, n, b.cent.as<float>(), b.tri_inst.as<uint32_t>(), bmin, bmax, bits, keys, vals);
    if (const int rc = sort_pairs(b, n, nb, st, err)) return rc;
    DCHK(hipMemcpyAsync(T.order.p, vals, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    if (n >= 2) {
        hipLaunchKernelGGL(karras_kernel, dim3(blocks_for(n - 1)), dim3(NT), 0, st, (int)n, keys, child, range, parent);
        hipLaunchKernelGGL(top_flag_kernel, dim3(blocks_for(n - 1)), dim3(NT), 0, st, (int)n, keys, range, shift, top);
    }
    hipLaunchKernelGGL(inst_root_kernel, dim3(blocks_for(2 * (size_t)n - 1)), dim3(NT), 0, st, (int)n, n_inst, keys, range, parent, top, shift, T.root.as<uint32_t>(), hdr);
    hipLaunchKernelGGL(top_ids_kernel, dim3(1), dim3(NT), 0, st, n - 1, top, k, T.top_ids.as<uint32_t>(), hdr);
    if (restructure) { // "device_bvh_opt" rounds on the object-space boxes, inside the instances
        if (const int rc = bvh2_boxes(b, n, vals, child, parent, st, err)) return rc;
        if (const int rc = restructure_bvh2(b, n, leaf_max, opt_rounds, child, parent, top, T.pos.as<uint32_t>(), range, st, err)) return rc;
    } else
        hipLaunchKernelGGL(iota_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, n, T.pos.as<uint32_t>());
    DCHK(hipGetLastError());
    uint32_t h[H_WORDS];
    const char* failed = "device BVH: the instance topology failed a structural bound (";
    T.k = k;
    T.graft = graft;
    T.skel_deep = false;
    T.n_skel = 0;
    if (graft) { // the skeleton walks the BVH2: only one that passed its bounds
        DCHK(hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, st));
        DCHK(hipStreamSynchronize(st));
        if (h[H_ERR]) { err = failed + std::to_string(h[H_ERR]) + ")"; return HJR_ERR_DEVICE; }
        if (const int rc = build_skeleton(b, n, n_inst, leaf_max, restructure, st, err)) return rc;
    }
    DCHK(hipEventRecord(b.ev1, st));
    DCHK(hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    DCHK(hipEventElapsedTime(&T.ms, b.ev0, b.ev1));
    if (h[H_ERR]) { err = failed + std::to_string(h[H_ERR]) + ")"; return HJR_ERR_DEVICE; }
    if (graft) // a commit reads pos, order, list and the skeleton only
        for (DevBuf* x : { &T.child, &T.range, &T.parent, &T.top, &T.top_ids, &T.root, &T.bounds }) x->release();
    T.valid = true;
    return HJR_OK;
}

int device_bvh_instances(DeviceBvh& b, const SceneCopy& sc, const float* M, const float* Mi, uint32_t n_inst, uint32_t leaf_max, uint32_t opt_rounds,
                         uint32_t tag, bool graft, const float* lights, size_t light_floats, hipStream_t st, DeviceBvhResult& r, std::string& err, DeviceMorph* dm)
{
    const uint32_t n = sc.n_triangles;
    std::vector<uint32_t> list; // the non-empty instances
    for (uint32_t i = 0; i < n_inst && i < sc.prim_offset.size(); i++)
        if ((i + 1 < n_inst && i + 1 < sc.prim_offset.size() ? sc.prim_offset[i + 1] : n) > sc.prim_offset[i]) list.push_back(i);
    auto ordinary = [&] { return device_bvh_build(b, sc, M, Mi, n_inst, leaf_max, opt_rounds, lights, light_floats, st, r, err, dm); };
    if (n == 0 || list.empty() || list.size() > HJR_TOP_MAX) return ordinary();
    r = DeviceBvhResult();
    if (!b.ev0) DCHK(hipEventCreate(&b.ev0));
    if (!b.ev1) DCHK(hipEventCreate(&b.ev1));
    if (!upload_scene(b, sc, st)) return fail_alloc(err);
    if (const int rc = prepare_morph(b, sc, dm, st, err)) return rc;
    const std::vector<float> xf = pack_transforms(M, Mi, n_inst);
    const size_t nn = n;
    const uint32_t nb = (uint32_t)((n + SORT_TILE - 1) / SORT_TILE);
    if (!b.xf.upload(xf.data(), xf.size() * 4, st) || !b.lights.upload(lights, light_floats * 4, st) || !b.hdr.reserve(H_WORDS * 4) ||
        !b.nodes.reserve(nn * HJR_NODE4_F4 * 16) || !b.tri_geom.reserve(nn * HJR_TRI_F4 * 16) || !b.tri_shade.reserve(nn * HJR_SHADE_F4 * 16) ||
        !b.tri_inst.reserve(nn * 4) || !b.part.reserve(SCAN_G * 4) || !b.leaf_box.reserve(nn * 32) || !b.inner_box.reserve(nn * 32) || !b.counter.reserve(nn * 4) ||
        !b.frontier[0].reserve(nn * sizeof(Front)) || !b.frontier[1].reserve(nn * sizeof(Front)) || !b.wide.reserve(nn * (sizeof(Wide) + 4)))
        return fail_alloc(err);
    DeviceBvh::Topology& T = b.topo;
    if (!T.valid || T.tag != tag || T.k != list.size() || T.graft != graft) {
        if (!b.box.reserve(nn * 32) || !b.cent.reserve(nn * 16) || !b.keys[0].reserve(nn * 8) || !b.keys[1].reserve(nn * 8) || !b.vals[0].reserve(nn * 4) ||
            !b.vals[1].reserve(nn * 4) || !b.hist.reserve(std::max<size_t>(1, (size_t)nb * 256 * 4)) || !b.node_count.reserve(nn * 4) || !b.node_cost.reserve(nn * 4))
            return fail_alloc(err);
        if (const int rc = build_topology(b, dm, n, n_inst, leaf_max, opt_rounds, graft, list, st, err)) return rc;
        T.tag = tag;
    }
    const uint32_t k = T.k;
    uint32_t* hdr = b.hdr.as<uint32_t>();
    if (graft && T.skel_deep) return ordinary(); // an instance tree deeper than the traversal stack
    // under device_bvh_graft no leaf boxes: the skeleton's boxes come from tri_geom
    LeafFlattenArgs fa = { flatten_args(b, dm, n, n_inst), nullptr, T.order.as<uint32_t>(), T.pos.as<uint32_t>(), b.tri_geom.as<float4>(),
                           graft ? nullptr : b.leaf_box.as<float4>() };
    if (graft) { // flatten, skeleton boxes, top tree, placement, cost: one host wait
        const uint32_t S = T.n_skel;
        NodeBoxArgs na = { n, S, T.skel_refs.as<float4>(), 1u, true, b.tri_geom.as<float4>(), b.stage.as<float4>(), T.skel_parent.as<uint32_t>(), b.counter.as<uint32_t>(), hdr };
        GraftTopArgs ga;
        ga.n = n; ga.k = k; ga.n_skel = S; ga.cap = (uint32_t)nn;
        ga.inst_ref = T.inst_ref.as<uint32_t>(); ga.inst_stat = T.inst_stat.as<uint32_t>();
        ga.stage = b.stage.as<float4>(); ga.geom = b.tri_geom.as<float4>();
        ga.box = T.top_box.as<float4>(); ga.nodes = b.nodes.as<float4>(); ga.hdr = hdr;
        DCHK(hipEventRecord(b.ev0, st));
        hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(64), 0, st, hdr);
        if (S) DCHK(hipMemsetAsync(b.counter.p, 0, (size_t)S * 4, st));
        hipLaunchKernelGGL(leaf_flatten_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, fa);
        if (S) hipLaunchKernelGGL(node_boxes_kernel, dim3(blocks_for(S)), dim3(NT), 0, st, na);
        hipLaunchKernelGGL(graft_top_kernel, dim3(1), dim3(NT), 0, st, ga);
        if (S) hipLaunchKernelGGL(graft_place_kernel, dim3(blocks_for((size_t)S * HJR_NODE4_F4)), dim3(NT), 0, st, S, (uint32_t)nn, b.stage.as<float4>(),
                                  b.counter.as<uint32_t>(), b.nodes.as<float4>(), hdr);
        launch_sah(b, b.nodes.as<float4>(), hdr + H_BASE, (uint32_t)nn, nullptr, st);
        DCHK(hipGetLastError());
        if (const int rc = read_header(b, st, r, "device BVH: the grafted instance tree", err)) return rc;
        if (r.stack_need > hjr::DEVICE_BVH_MAX_STACK) return ordinary(); // a chain-shaped top tree (nested instances)
        r.instances = k;
        return HJR_OK;
    }
    InstArgs a = { n, T.top.as<uint32_t>(), T.parent.as<uint32_t>(), T.child.as<uint2>(), b.counter.as<uint32_t>(), hdr, b.leaf_box.as<float4>(), b.inner_box.as<float4>() };
    DCHK(hipEventRecord(b.ev0, st));
    hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(64), 0, st, hdr);
    if (n >= 2) DCHK(hipMemsetAsync(b.counter.p, 0, (size_t)(n - 1) * 4, st));
    hipLaunchKernelGGL(leaf_flatten_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, fa);
    hipLaunchKernelGGL(inst_boxes_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, a);
    if (k >= 2) {
        TopArgs ta;
        ta.n = n; ta.n_inst = n_inst; ta.k = k;
        ta.list = T.list.as<uint32_t>(); ta.root = T.root.as<uint32_t>(); ta.top = T.top.as<uint32_t>(); ta.top_ids = T.top_ids.as<uint32_t>();
        ta.child = T.child.as<uint2>(); ta.range = T.range.as<uint2>(); ta.parent = T.parent.as<uint32_t>();
        ta.leaf_box = b.leaf_box.as<float4>(); ta.inner_box = b.inner_box.as<float4>(); ta.hdr = hdr;
        hipLaunchKernelGGL(inst_top_kernel, dim3(1), dim3(NT), 0, st, ta);
    }
    DCHK(hipGetLastError());
    CollapseArgs ca;
    ca.child = T.child.as<uint2>(); ca.range = T.range.as<uint2>();
    ca.leaf_box = b.leaf_box.as<float4>(); ca.inner_box = b.inner_box.as<float4>();
    ca.leaf_pos = T.pos.as<uint32_t>();
    ca.leaf_max = leaf_max; ca.cap = (uint32_t)nn; ca.hdr = hdr;
    ca.top = T.top.as<uint32_t>(); ca.inst_stat = nullptr;
    const int rc = collapse_and_cost(b, ca, n, nn, st, r, "device BVH: the instance tree", err);
    if (rc != HJR_OK && r.too_deep) return ordinary(); // a chain-shaped top tree (nested instances): the Morton tree over all triangles
    if (rc == HJR_OK) r.instances = k;
    return rc;
}

} // namespace hjr
