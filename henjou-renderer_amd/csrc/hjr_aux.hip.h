// The small kernels around the render kernels: cost-ordered tile list, chunk-sum finalisation, firefly clamp, adaptive sampling's rule 11
// and tile filter.  Included by hjr_render.hip only (non-template __global__ functions: one translation unit).
#pragma once
#include "hjr_traverse.hip.h"

// ---- cost-ordered tile list.  The frame ends when the slowest work item ends, and an item (8 samples of one pixel, each up
// to 10 bounces, strictly sequential) can run for milliseconds: with plain scanline order the tail of the launch is whatever
// the last tiles happen to cost (5 ms on a 64 x 64 frame, 15 % of an 18 ms launch when the frame is split over 8 GPUs).
// One wave per owned tile casts the 64 pixel-centre rays (no RNG), classifies the tile by its costliest first hit
// (3 = glass, 2 = metallic, 1 = other surface, 0 = background or light) and the tiles are handed out class 3 first, background
// last: longest-processing-time-first scheduling, and waves whose lanes behave alike.  Only the ORDER of the work changes;
// every pixel is computed exactly as before.
template <int WIDTH>
__global__ void __launch_bounds__(64) hjr_classify_tiles_kernel(const KParams P)
{
    TileStack stack = hjr_tile_stack();
    uint32_t n_cls[4] = { 0u, 0u, 0u, 0u }; // per block; one atomic per class at the end (32 k atomics on four words cost 0.4 ms)
    for (uint32_t idx = blockIdx.x; idx < P.n_owned_tiles; idx += gridDim.x) {
        const uint32_t tile = idx * P.world + P.rank;
        uint32_t tx, ty;
        hjr_tile_xy(tile, P.tiles_x, &tx, &ty);
        const uint32_t wx = tx * HJR_TILE + (threadIdx.x & 7u), wy = ty * HJR_TILE + (threadIdx.x >> 3); // in the work rectangle (the window's tile grid)
        const uint32_t px = wx + (P.win_word & 0x1fffu), py = wy + (P.win_word >> 13);                     // in the frame: the centre ray is the frame's
        uint32_t cls = 0;
        if (wx < P.work_w && wy < P.work_h) {
            const float W = (float)P.width, H = (float)P.height;
            const float u = (2.0f * ((float)px + 0.5f) - W) / H, v = (2.0f * ((float)py + 0.5f) - H) / H;
            const f3 cd = V(P.cam_dir[0], P.cam_dir[1], P.cam_dir[2]), cu = V(P.cam_up[0], P.cam_up[1], P.cam_up[2]);
            const f3 cr = V(P.cam_right[0], P.cam_right[1], P.cam_right[2]);
            const f3 d = normalize(cd * P.cam_f + cr * u + cu * v);
            Hit h;
            Counters cnt; cnt.box = cnt.tri = 0;
            if (traverse<false, false, WIDTH, 64, TileStack>(P.nodes, P.tri_geom, V(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]), d, 0.001f, 1e16f, h, stack, cnt)) {
                const float4* m = P.materials + f2bits(P.tri_geom[h.k * HJR_TRI_F4 + 2].z) * HJR_MAT_F4;
                const float4 m0 = m[0], m3 = m[3];
                cls = f2bits(m3.x) != 0 ? 0u : (f2bits(m3.y) != 0 ? 3u : (m0.w > 0.5f ? 2u : 1u));
            }
        }
        const uint32_t tcls = __ballot(cls == 3u) ? 3u : (__ballot(cls == 2u) ? 2u : (__ballot(cls == 1u) ? 1u : 0u));
        if (threadIdx.x == 0) P.tile_class[idx] = tcls;
        n_cls[0] += tcls == 0u; n_cls[1] += tcls == 1u; n_cls[2] += tcls == 2u; n_cls[3] += tcls == 3u;
    }
    if (threadIdx.x < 4u && n_cls[threadIdx.x]) atomicAdd(&P.tile_count[threadIdx.x], n_cls[threadIdx.x]);
}
__global__ void __launch_bounds__(256) hjr_order_tiles_kernel(const KParams P)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    const bool live = idx < P.n_owned_tiles;
    const uint32_t cls = live ? P.tile_class[idx] : 0xffffffffu;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t pos = 0;
    for (uint32_t c = 0; c < 4u; c++) { // wave-aggregated scatter: one atomic per wave and class
        const unsigned long long m = __ballot(cls == c);
        if (m == 0ull) continue;
        uint32_t base = 0;
        if (lane == (uint32_t)(__ffsll((long long)m) - 1)) base = atomicAdd(&P.tile_count[4 + c], (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, __ffsll((long long)m) - 1);
        if (cls == c) {
            uint32_t first = 0;
            for (uint32_t k = 3u; k > c; k--) first += P.tile_count[k];
            pos = first + base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        }
    }
    if (live) P.tile_order_w[pos] = idx * P.world + P.rank;
}

// From the second frame of a sequence on, the tiles are ordered by what they actually cost in the previous frame (closest-hit
// rays per sample) inside their first-hit class: a counting sort over 64 keys in two kernels; the order inside a key is arbitrary.
HD uint32_t cost_bucket(uint32_t cls, uint32_t cost, uint32_t cost_div)
{
    // key = (first-hit class, measured rays per sample in steps of 1/2): the class keeps waves of like materials together in
    // time (3 % at N = 1), the cost orders the tiles inside a class so that the last items of a class are its cheapest
    const uint32_t b = (uint32_t)(((unsigned long long)cost * 2ull) / cost_div);
    return (cls & 3u) * 16u + (b > 15u ? 15u : b);
}
__global__ void __launch_bounds__(256) hjr_cost_hist_kernel(const KParams P)
{
    __shared__ uint32_t h[64];
    if (threadIdx.x < 64u) h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx < P.n_owned_tiles) {
        const uint32_t b = cost_bucket(P.tile_class[idx], P.tile_cost[idx], P.cost_div);
        P.tile_bucket[idx] = b;
        atomicAdd(&h[b], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 64u && h[threadIdx.x]) atomicAdd(&P.cost_hist[threadIdx.x], h[threadIdx.x]);
}
__global__ void __launch_bounds__(256) hjr_cost_scatter_kernel(const KParams P)
{
    __shared__ uint32_t h[64], base[64];
    if (threadIdx.x < 64u) h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    const bool live = idx < P.n_owned_tiles;
    uint32_t b = 0, rank_in_block = 0;
    if (live) { b = P.tile_bucket[idx]; rank_in_block = atomicAdd(&h[b], 1u); P.tile_cost[idx] = 0u; } // zeroed for this frame's sums
    __syncthreads();
    if (threadIdx.x < 64u) {
        uint32_t first = 0;
        for (uint32_t k = 63u; k > threadIdx.x; k--) first += P.cost_hist[k]; // expensive buckets first
        base[threadIdx.x] = h[threadIdx.x] ? first + atomicAdd(&P.cost_hist[64u + threadIdx.x], h[threadIdx.x]) : 0u;
    }
    __syncthreads();
    if (live) P.tile_order_w[base[b] + rank_in_block] = idx * P.world + P.rank;
}

// variance of a pixel's mean from the statistic of its chunk sums (DESIGN.md §4 rule 7)
__device__ inline float hjr_variance_of_mean(float S1, float S2, uint32_t m_chunks, uint32_t granule, uint32_t n_samples)
{
    if (m_chunks < 2u) return HJR_VARIANCE_UNKNOWN;
    const float m = (float)m_chunks;
    const float q = fmaxf(m * S2 - S1 * S1, 0.0f);
    return (q / (m * (m - 1.0f))) / ((float)granule * (float)n_samples);
}
// frames of a single chunk (no chunk sums exist: the render kernel wrote the means itself): every owned pixel is UNKNOWN
__global__ void __launch_bounds__(256) hjr_fill_var_kernel(const KParams P, float* __restrict__ aov_var)
{
    const size_t n_slots = (size_t)P.n_owned_tiles * 64u;
    for (size_t sl = (size_t)blockIdx.x * blockDim.x + threadIdx.x; sl < n_slots; sl += (size_t)gridDim.x * blockDim.x) {
        uint32_t x, y;
        if (!hjr_slot_xy(sl, P.rank, P.world, P.tiles_x, P.work_w, P.work_h, &x, &y)) continue;
        aov_var[P.packed ? sl : (size_t)y * P.work_w + x] = HJR_VARIANCE_UNKNOWN;
    }
}

// ---- chunk sums -> pixel means (DESIGN.md §4 rules 4 - 7, §6.2).  Adds the chunk sums of every owned pixel in chunk order and scales by
// 1/n: a fixed summation tree, so the frame is bitwise independent of which lane/wave/GPU rendered which chunk.  Streaming kernel: one lane
// per pixel of an owned tile, coalesced float4 loads ([chunk][owned tile][64] layout), one float4 store per AOV.  The summation is written
// ONCE, here; the flags only select what surrounds it, at compile time, so an instantiation holds no code of a feature it does not have:
//   PASS      a sample pass (hjr_params.sample_begin / sample_end, rule 5): chunks [chunk0, chunk0 + pass_chunks) instead of [0, n_chunks),
//             added to the running sum of the frame's earlier passes (+0.0f on its first pass), which goes back unless this is the frame's
//             last pass; the mean is over sample_end samples instead of spp.  Chunk by chunk this is the one-shot summation, so the pass
//             that ends at spp writes the one-shot frame's bits.
//   ADAPTIVE  adaptive sampling (hjr_set_adaptive, rule 6; implies PASS): one wave per owned tile (the grid stride is a multiple of 64 and
//             n_slots is one, so the 64 lanes of a wave always hold the 64 pixels of one tile and leave the loop together).  A STOPPED tile
//             (ad_state = n_tile) reads no chunk sum (the render kernel left its slots alone: they are stale) and keeps its mean over
//             n_tile samples.  After a pass that decides, every ACTIVE tile (ad_state 0) evaluates the stopping rule: IEEE fp32 + - * /
//             sqrt max as written (this translation unit is built with correctly rounded divide / sqrt and without contraction) and a
//             fixed xor butterfly, so numpy float32 restates it bit for bit.  Out-of-image lanes of an edge tile are predicated, never
//             skipped, until after the butterfly: they carry e = 0 into it.  Every pass writes every owned pixel of every requested AOV.
//   VAR       the variance AOV (hjr_render_var, rule 7): one more float store per pixel.
// The statistic (S1, S2) over y = (c.x + c.y) + c.z of the colour sums exists iff ADAPTIVE || VAR, and is over the FULL chunks a pixel has
// received (k < spp / chunk_spp), in chunk order from +0.0f; the partial last chunk goes into the colour only.  A pass keeps it per owned
// pixel in P.stat.
template <bool PASS, bool ADAPTIVE, bool VAR>
__global__ void __launch_bounds__(256) hjr_finalize_kernel(const KParams P, float* __restrict__ aov_var)
{
    static_assert(PASS || !ADAPTIVE, "adaptive sampling acts on sample passes");
    constexpr bool STAT = ADAPTIVE || VAR;
    const size_t n_slots = (size_t)P.n_owned_tiles * 64u; // chunk-sum slots per chunk: 64 per owned tile
    const uint32_t k_begin = PASS ? P.chunk0 : 0u, k_end = PASS ? P.chunk0 + P.pass_chunks : P.n_chunks; // (part_* are offset by -chunk0 chunks: see KParams)
    const uint32_t n_full = P.spp / P.chunk_spp;
    const uint32_t n_frame = PASS ? P.sample_end : P.spp;
    const bool run_load = PASS && P.run_load, run_store = PASS && P.run_store;
    for (size_t sl = (size_t)blockIdx.x * blockDim.x + threadIdx.x; sl < n_slots; sl += (size_t)gridDim.x * blockDim.x) {
        uint32_t x, y;
        const bool inside = hjr_slot_xy(sl, P.rank, P.world, P.tiles_x, P.work_w, P.work_h, &x, &y);
        if constexpr (!ADAPTIVE) { if (!inside) continue; }
        uint32_t n_tile = 0u; // (wave-uniform) 0: the tile is active
        if constexpr (ADAPTIVE) n_tile = run_load ? P.ad_state[sl >> 6] : 0u;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a;
        float2 s = make_float2(0.0f, 0.0f);
        if (inside && run_load) {
            a = P.run_color[sl];
            if (P.aov_albedo) b = P.run_albedo[sl];
            if (P.aov_normal) c = P.run_normal[sl];
            if constexpr (STAT) s = P.stat[sl];
        }
        if (n_tile == 0u) {
            if (inside) {
                for (uint32_t k = k_begin; k < k_end; k++) {
                    const float4 v = P.part_color[(size_t)k * n_slots + sl];
                    a.x = a.x + v.x; a.y = a.y + v.y; a.z = a.z + v.z;
                    if constexpr (STAT) if (k < n_full) { const float yk = (v.x + v.y) + v.z; s.x = s.x + yk; s.y = s.y + yk * yk; }
                    if (P.aov_albedo) { const float4 w = P.part_albedo[(size_t)k * n_slots + sl]; b.x = b.x + w.x; b.y = b.y + w.y; b.z = b.z + w.z; }
                    if (P.aov_normal) { const float4 w = P.part_normal[(size_t)k * n_slots + sl]; c.x = c.x + w.x; c.y = c.y + w.y; c.z = c.z + w.z; }
                }
                if (run_store) {
                    P.run_color[sl] = make_float4(a.x, a.y, a.z, 0.0f);
                    if (P.aov_albedo) P.run_albedo[sl] = make_float4(b.x, b.y, b.z, 0.0f);
                    if (P.aov_normal) P.run_normal[sl] = make_float4(c.x, c.y, c.z, 0.0f);
                    if constexpr (STAT) P.stat[sl] = s;
                }
            }
            if constexpr (ADAPTIVE) {
                if (P.ad_decide) { // (wave-uniform branch: all 64 lanes take the butterfly)
                    const float n = (float)P.sample_end, m = (float)(P.sample_end / P.chunk_spp);
                    const float q = fmaxf(m * s.y - s.x * s.x, 0.0f);
                    const float e = sqrtf(q / (m - 1.0f)) / (s.x + HJR_ADAPTIVE_EPS * n);
                    float v = inside ? e : 0.0f;
                    for (int k = 32; k >= 1; k >>= 1) v = v + __shfl_xor(v, k, 64);
                    if (v <= P.ad_threshold * 64.0f) n_tile = P.sample_end;
                }
                if ((threadIdx.x & 63u) == 0u) {
                    P.ad_state[sl >> 6] = n_tile;
                    if (n_tile == 0u) atomicAdd(&P.ad_state[P.n_owned_tiles], 1u);
                }
            }
        }
        if constexpr (ADAPTIVE) { if (!inside) continue; } // (after the butterfly)
        const uint32_t n_mean = n_tile ? n_tile : n_frame; // the samples the written mean is over
        const float inv = 1.0f / (float)n_mean;
        const size_t pix = P.packed ? sl : (size_t)y * P.work_w + x;
        P.aov_color[pix] = make_float4(a.x * inv, a.y * inv, a.z * inv, 1.0f);
        if (P.aov_albedo) P.aov_albedo[pix] = make_float4(b.x * inv, b.y * inv, b.z * inv, 1.0f);
        if (P.aov_normal) P.aov_normal[pix] = make_float4(c.x * inv, c.y * inv, c.z * inv, 1.0f);
        if constexpr (VAR) aov_var[pix] = hjr_variance_of_mean(s.x, s.y, n_mean / P.chunk_spp, P.chunk_spp, n_mean);
    }
}

// ---- firefly clamp (option "firefly_clamp", DESIGN.md §4 rules 9 and 10; the rules are stated in include/henjou_hip.h).  Runs BEHIND
// hjr_finalize_kernel<false, false, VAR> on a one-shot frame of m = spp / chunk_spp >= 4 full chunks: the plain frame, its albedo, normal and
// variance stand as that kernel wrote them (the summation stays written once, there), and this kernel rewrites the COLOUR of exactly the pixels
// that have a scaled chunk, so every other pixel keeps the plain frame's bits by construction.  What it adds is a different sum: every chunk
// whose y = (c.x + c.y) + c.z exceeds kappa x the lower median of the pixel's full chunks (+ eps x granule) is scaled down to that limit.
// One lane per pixel of an owned tile, whole waves per tile (n_slots and the grid stride are multiples of 64).  Stream 1 puts the y of the
// full chunks into the lane's LDS column (ys[k * BLOCK]: conflict-free, at most 64 x BLOCK floats; no per-lane array, no scratch) and keeps
// their maximum; the median is the y of rank (m - 1) / 2 in the order (y, k), found by counting, O(m^2) LDS reads; stream 2, entered only by
// waves with a lane over its limit, reads the colour sums again (the pixel's 16 m bytes were read a moment ago: L2) and adds them scaled, in
// chunk order from +0.0f.  The scaled (pixel, chunk) pairs are counted per lane, added over the wave, one integer atomic per wave.
// fp32 as written, correctly rounded divide, no contraction (this translation unit's flags): numpy float32 restates it bit for bit.
// The flags select what surrounds that, at compile time, as in hjr_finalize_kernel; the one-shot instantiation holds none of it:
//   PASS      option "firefly_clamp_passes" (rule 10): behind hjr_finalize_kernel<true, ADAPTIVE, VAR> on a sample pass that ends at
//             n = sample_end with m_n = n / chunk_spp >= 4.  P.part_color is the base of the colour chunk sums the context keeps for the whole
//             progressive frame; chunks [0, m_n) are streamed, and the partial chunk m_n when n = spp (r_n > 0 only then).  The mean is over n.
//   ADAPTIVE  (implies PASS) the pass of an adaptive frame.  A STOPPED tile (ad_state = n_tile, as the finalize kernel left it) is clamped
//             over its own chunks [0, n_tile / chunk_spp) with n = n_tile, or left alone when those are fewer than 4: the slots behind them
//             are stale and never read.  With P.ad_decide (the finalize kernel ran with 0) every ACTIVE tile takes rule 6's decision here,
//             from the statistic of the CLAMPED sums, y' = (c.x s + c.y s) + c.z s with the products of the colour sum: a lane over its limit
//             adds them in stream 2, any other lane has s = 1 throughout and adds its LDS column (y' = y to the bit).  All 64 lanes of the
//             wave reach the butterfly, out-of-image lanes with e = 0; a tile that stops gets ad_state = n and leaves the active count.
template <uint32_t BLOCK, bool PASS, bool ADAPTIVE>
__global__ void __launch_bounds__(BLOCK) hjr_firefly_kernel(const KParams P, const float kappa, unsigned long long* __restrict__ n_clamped)
{
    static_assert(PASS || !ADAPTIVE, "adaptive sampling acts on sample passes");
    float* const ys = reinterpret_cast<float*>(hjr_smem) + threadIdx.x;
    const size_t n_slots = (size_t)P.n_owned_tiles * 64u;
    const uint32_t g = P.chunk_spp, n_pass = PASS ? P.sample_end : P.spp;
    uint32_t n = n_pass, m = n / g, r = n - m * g; // samples of the mean, full chunks, samples of the partial last chunk (chunk m, if r > 0)
    uint32_t want = (m - 1u) / 2u;                 // rank of the lower median
    float inv = 1.0f / (float)n;
    uint32_t n_scaled = 0u;
    for (size_t sl = (size_t)blockIdx.x * BLOCK + threadIdx.x; sl < n_slots; sl += (size_t)gridDim.x * BLOCK) {
        uint32_t x, y;
        const bool inside = hjr_slot_xy(sl, P.rank, P.world, P.tiles_x, P.work_w, P.work_h, &x, &y);
        bool deciding = false; // (wave-uniform)
        if constexpr (ADAPTIVE) {
            const uint32_t n_tile = P.ad_state[sl >> 6];
            n = n_tile ? n_tile : n_pass; m = n / g; r = n - m * g;
            if (m < 4u) continue; // the rule does not act on this tile
            want = (m - 1u) / 2u; inv = 1.0f / (float)n;
            deciding = P.ad_decide != 0u && n_tile == 0u;
        }
        float lim = 0.0f, lim_r = 0.0f;
        bool over = false;
        if (inside) {
            float y_max = -INFINITY;
            for (uint32_t k = 0; k < m; k++) {
                const float4 v = P.part_color[(size_t)k * n_slots + sl];
                const float yk = (v.x + v.y) + v.z;
                ys[k * BLOCK] = yk;
                y_max = fmaxf(y_max, yk);
            }
            float med = 0.0f;
            for (uint32_t k = 0; k < m; k++) {
                const float yk = ys[k * BLOCK];
                uint32_t below = 0u;
                for (uint32_t j = 0; j < m; j++) { const float yj = ys[j * BLOCK]; below += (yj < yk || (yj == yk && j < k)) ? 1u : 0u; }
                if (below == want) med = yk;
            }
            lim = kappa * med + HJR_FIREFLY_EPS * (float)g;
            over = y_max > lim;
            if (r) {
                lim_r = lim * ((float)r / (float)g);
                const float4 v = P.part_color[(size_t)m * n_slots + sl];
                over = over || (v.x + v.y) + v.z > lim_r;
            }
        }
        if (!deciding && !__any(over)) continue; // (wave-uniform)
        float S1 = 0.0f, S2 = 0.0f; // ADAPTIVE: the statistic of the clamped sums over the full chunks
        if (over) {
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const uint32_t k_end = PASS ? m + (r ? 1u : 0u) : P.n_chunks;
            for (uint32_t k = 0; k < k_end; k++) {
                const float4 v = P.part_color[(size_t)k * n_slots + sl];
                const float yk = (v.x + v.y) + v.z, L = k < m ? lim : lim_r;
                const bool scale = yk > L;
                const float s = scale ? L / yk : 1.0f;
                a.x = a.x + v.x * s; a.y = a.y + v.y * s; a.z = a.z + v.z * s;
                n_scaled += scale ? 1u : 0u;
                if constexpr (ADAPTIVE) if (k < m) { const float yc = (v.x * s + v.y * s) + v.z * s; S1 = S1 + yc; S2 = S2 + yc * yc; } // (the three products above)
            }
            P.aov_color[P.packed ? sl : (size_t)y * P.work_w + x] = make_float4(a.x * inv, a.y * inv, a.z * inv, 1.0f);
        }
        if constexpr (ADAPTIVE) {
            if (!deciding) continue;
            if (inside && !over)
                for (uint32_t k = 0; k < m; k++) { const float yk = ys[k * BLOCK]; S1 = S1 + yk; S2 = S2 + yk * yk; }
            const float nf = (float)n, mf = (float)m;
            const float q = fmaxf(mf * S2 - S1 * S1, 0.0f);
            const float e = sqrtf(q / (mf - 1.0f)) / (S1 + HJR_ADAPTIVE_EPS * nf);
            float v = inside ? e : 0.0f;
            for (int k = 32; k >= 1; k >>= 1) v = v + __shfl_xor(v, k, 64);
            if (v <= P.ad_threshold * 64.0f && (threadIdx.x & 63u) == 0u) {
                P.ad_state[sl >> 6] = n;
                atomicSub(&P.ad_state[P.n_owned_tiles], 1u); // (the finalize kernel counted the tile as active)
            }
        }
    }
    for (int k = 32; k >= 1; k >>= 1) n_scaled += (uint32_t)__shfl_xor((int)n_scaled, k, 64);
    if ((threadIdx.x & 63u) == 0u && n_scaled) atomicAdd(n_clamped, (unsigned long long)n_scaled);
}

// ---- adaptive sampling that counts the temporal history (option "adaptive_temporal", DESIGN.md §4 rule 11; stated in include/henjou_hip.h).
// Runs BEHIND hjr_finalize_kernel<true, true, VAR> on a deciding pass of an adaptive frame that has a prior (hjr_temporal_prior_kernel,
// csrc/hjr_temporal.hip.h: (lp, vp, al, 0) per pixel in frame layout); the finalize kernel ran with ad_decide 0, so every tile that was
// active stands as active (ad_state 0, counted), its raw statistic (S1, S2) is in P.stat and every AOV is written.  One wave per owned tile
// (n_slots and the grid stride are multiples of 64); a stopped tile's wave leaves at once.  Per pixel of an active tile, n = sample_end,
// g = chunk_spp, m = n / g, fp32 as written (correctly rounded divide and sqrt, no contraction: this translation unit's flags):
//     e6 = sqrtf(fmaxf(m S2 - S1 S1, 0) / (m - 1)) / (S1 + HJR_ADAPTIVE_EPS n)                       (rule 6's e: the expression of hjr_finalize_kernel)
//     if al < 1:   lc = S1 / n;   vc = hjr_variance_of_mean(S1, S2, m, g, n);   om = 1 - al;   va = (om om) vp + (al al) vc;
//                  la = lp + (lc - lp) al;   ea = sqrtf(va) / (fmaxf(la, 0) + HJR_ADAPTIVE_EPS);   e = fminf(ea, e6)     (a NaN ea gives e6)
//     else         e = e6
// Out-of-image lanes of an edge tile carry e = 0 into rule 6's xor butterfly; the tile stops iff the sum <= noise_threshold x 64, and lane 0
// then writes ad_state = n and takes the tile out of the active count.  e <= e6 per pixel and float addition is monotone, so a tile that
// rule 6 stops on this statistic stops here too.  The prior is an argument of its own: KParams does not grow.
__global__ void __launch_bounds__(256) hjr_adaptive_temporal_kernel(const KParams P, const float4* __restrict__ prior)
{
    const size_t n_slots = (size_t)P.n_owned_tiles * 64u;
    const uint32_t n = P.sample_end, g = P.chunk_spp, m = n / g;
    const float nf = (float)n, mf = (float)m;
    for (size_t sl = (size_t)blockIdx.x * blockDim.x + threadIdx.x; sl < n_slots; sl += (size_t)gridDim.x * blockDim.x) {
        if (P.ad_state[sl >> 6] != 0u) continue; // (wave-uniform) stopped before this pass
        uint32_t x, y;
        const bool inside = hjr_slot_xy(sl, P.rank, P.world, P.tiles_x, P.work_w, P.work_h, &x, &y);
        float e = 0.0f;
        if (inside) {
            const float2 s = P.stat[sl];
            const float q = fmaxf(mf * s.y - s.x * s.x, 0.0f);
            const float e6 = sqrtf(q / (mf - 1.0f)) / (s.x + HJR_ADAPTIVE_EPS * nf);
            const float4 pr = prior[(size_t)y * P.work_w + x]; // (lp, vp, al, 0)
            e = e6;
            if (pr.z < 1.0f) {
                const float lc = s.x / nf;
                const float vc = hjr_variance_of_mean(s.x, s.y, m, g, n);
                const float om = 1.0f - pr.z;
                const float va = (om * om) * pr.y + (pr.z * pr.z) * vc;
                const float la = pr.x + (lc - pr.x) * pr.z;
                const float ea = sqrtf(va) / (fmaxf(la, 0.0f) + HJR_ADAPTIVE_EPS);
                e = fminf(ea, e6);
            }
        }
        float v = e;
        for (int k = 32; k >= 1; k >>= 1) v = v + __shfl_xor(v, k, 64);
        if (v <= P.ad_threshold * 64.0f && (threadIdx.x & 63u) == 0u) {
            P.ad_state[sl >> 6] = n;
            atomicSub(&P.ad_state[P.n_owned_tiles], 1u); // (the finalize kernel counted the tile as active)
        }
    }
}

// The launch's tile list without the stopped tiles: a STABLE compaction of ad_src (the cost order hjr_order_tiles_kernel /
// hjr_cost_scatter_kernel just produced, or the plain round-robin order when there is none), so the expensive-first order survives and the
// result is the same for the same input.  At most 129 600 tiles (4K): one workgroup walks the list in steps of 1024 with a ballot per wave
// and a scan over the 16 wave counts in LDS.
__global__ void __launch_bounds__(1024) hjr_filter_tiles_kernel(const KParams P)
{
    __shared__ uint32_t wave_n[16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t done = 0; // tiles kept so far (the same in every thread)
    for (uint32_t base = 0; base < P.n_owned_tiles; base += 1024u) {
        const uint32_t idx = base + threadIdx.x;
        const bool live = idx < P.n_owned_tiles;
        const uint32_t tile = live ? (P.ad_src ? P.ad_src[idx] : idx * P.world + P.rank) : 0u;
        const bool keep = live && P.ad_state[tile / P.world] == 0u;
        const unsigned long long mk = __ballot(keep);
        if (lane == 0u) wave_n[wave] = (uint32_t)__popcll(mk);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 16u; w++) { const uint32_t nw = wave_n[w]; before += w < wave ? nw : 0u; total += nw; }
        if (keep) P.ad_list[done + before + (uint32_t)__popcll(mk & ((1ull << lane) - 1ull))] = tile;
        done += total;
        __syncthreads(); // wave_n is rewritten by the next step
    }
}
