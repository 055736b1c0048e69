// Ray-batch test hook (hjr_trace_rays, include/henjou_hip.h): kernels that hand caller-chosen rays to the traversal of the render kernels.
// Nothing of the traversal or of a kernel's set-up is restated here: the kernels run hjr_render_kernel's prologue (hjr_kernel.hip.h::kernel_prologue:
// the LaneStack of the layout, the scene staging, the BVH4 `top` copy) and call traverse<> / traverse_fused<> of hjr_traverse.hip.h as they are.  Two translation units
// instantiate them: hjr_launch_trace.hip with the exact flags and hjr_launch_fast_trace.hip with the Makefile's FASTFLAGS (HJR_TRACE_FAST_BUILD),
// which is how "the traversal and the triangle test are the same operations in every build" is checked ray by ray.
// Included by those two units and by hjr_util.hip (the entry point) only: no render kernel sees this header.
#pragma once
#include "hjr_launch.hip.h"

struct TraceArgs {
    KParams P;                   // scene tables and the layout's launch parameters, as plan_launch set them
    const hjr_ray* shadow;
    const hjr_ray* closest;
    hjr_ray_result* out;         // uploaded with status = HJR_TRACE_STATUS_UNTRACED; a resolved pair overwrites its record
    uint32_t n;
    uint32_t round_cap;          // fused path: rounds a wave may run
    unsigned int* next;          // fused path: next pair to hand out
    unsigned long long* n_over;  // stack pushes that went to the HBM overflow, summed over the grid
};

// the lane's stack and scene pointers: hjr_render_kernel's own prologue, called as that kernel calls it (COUNT = true: overflow pushes are counted)
template <int BLOCK, bool LDSBVH, bool STACK16, int WIDTH> struct TraceLayout {
    typedef typename std::conditional<STACK16, uint16_t, uint32_t>::type SE;
    typedef LaneStack<SE, BLOCK, !LDSBVH, true, LDSBVH> ST;
    static HD void setup(const KParams& P, ST& stack, const float4*& nodes, const float4*& tris)
    {
        const float4 *mats, *lights;
        kernel_prologue<BLOCK, LDSBVH, WIDTH == 4>(P, stack, lds_behind_stacks<SE, BLOCK>(LDSBVH ? P.stack_depth : P.stack_lds_entries), nodes, tris, mats, lights);
    }
    static HD void flush_overflow(const ST& stack, unsigned long long* n_over)
    {
        const unsigned long long v = wave_sum(stack.n_over);
        if ((threadIdx.x & 63u) == 0u && v) atomicAdd(n_over, v);
    }
};

HD void trace_store(hjr_ray_result* out, uint32_t i, bool occluded, const Hit& h, uint32_t status)
{
    const bool hit = h.prim != 0xffffffffu;
    hjr_ray_result r;
    r.occluded = occluded ? 1u : 0u;
    r.prim = h.prim;
    r.k = hit ? h.k : 0u;
    r.t = hit ? h.t : 0.0f; r.b1 = hit ? h.b1 : 0.0f; r.b2 = hit ? h.b2 : 0.0f;
    r.status = status; r.pad = 0u;
    out[i] = r;
}

// HJR_TRACE_STANDALONE: traverse<ANY = true> for the shadow ray, traverse<ANY = false> for the closest-hit ray (the loop of MIS' ray_trace and of
// the tile classifier), tmin 0.001, the closest-hit ray's far end 1e16 as in ray_trace.  FAST only tags the symbol, like hjr_render_kernel's.
template <int BLOCK, bool LDSBVH, bool STACK16, int WIDTH, bool FAST>
__global__ void __launch_bounds__(BLOCK, (LDSBVH ? 1 : HJR_MIN_WAVES)) hjr_trace_standalone_kernel(const TraceArgs A)
{
    typedef TraceLayout<BLOCK, LDSBVH, STACK16, WIDTH> L;
    typename L::ST stack;
    const float4 *nodes, *tris;
    L::setup(A.P, stack, nodes, tris);
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < A.n; i += gridDim.x * BLOCK) {
        const hjr_ray s = A.shadow[i], c = A.closest[i];
        Counters cnt; cnt.box = cnt.tri = 0;
        Hit h;
        bool occluded = false;
        if (s.valid) occluded = traverse<true, false, WIDTH, BLOCK, typename L::ST>(nodes, tris, V(s.o[0], s.o[1], s.o[2]), V(s.d[0], s.d[1], s.d[2]), 0.001f, s.tmax, h, stack, cnt);
        h.prim = 0xffffffffu;
        if (c.valid) traverse<false, false, WIDTH, BLOCK, typename L::ST>(nodes, tris, V(c.o[0], c.o[1], c.o[2]), V(c.d[0], c.d[1], c.d[2]), 0.001f, 1e16f, h, stack, cnt);
        trace_store(A.out, i, occluded, h, HJR_TRACE_STATUS_OK);
    }
    L::flush_overflow(stack, A.n_over);
}

// HJR_TRACE_FUSED: traverse_fused with the layout's production CARRY and the launch's node_min, driven like the rounds of hjr_render_kernel: a
// lane whose pair is resolved takes the next one (one atomic per wave and round, ballot + mbcnt prefix), a lane whose call returned "in
// flight" keeps its pair and resumes next to the other lanes' fresh pairs.  A wave that has run round_cap rounds marks the pairs it still
// holds HJR_TRACE_STATUS_ROUND_CAP and leaves.
template <int BLOCK, bool LDSBVH, bool STACK16, int WIDTH, bool FAST>
__global__ void __launch_bounds__(BLOCK, (LDSBVH ? 1 : HJR_MIN_WAVES)) hjr_trace_fused_kernel(const TraceArgs A)
{
    typedef TraceLayout<BLOCK, LDSBVH, STACK16, WIDTH> L;
    typename L::ST stack;
    const float4 *nodes, *tris;
    L::setup(A.P, stack, nodes, tris);
    const uint32_t lane = threadIdx.x & 63u;
    bool inflight = false, have = false, dry = false; // dry is wave-uniform
    uint32_t mine = 0u;
    hjr_ray s, c;
    s.valid = c.valid = 0u; s.tmax = 0.0f;
    for (int k = 0; k < 3; k++) { s.o[k] = s.d[k] = c.o[k] = c.d[k] = 0.0f; }
    bool occluded = false;
    Hit h; h.prim = 0xffffffffu; h.t = 0.0f; h.b1 = h.b2 = 0.0f; h.k = 0u;
    TravCarry tc; tc.cur = HJR_TRAV_DONE; tc.sp = 0; tc.phase = 2;
    for (uint32_t round = 0;; round++) {
        const unsigned long long m = __ballot(!have);
        if (m && !dry) {
            const uint32_t want = (uint32_t)__popcll(m);
            const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            uint32_t base = 0u;
            if (lane == 0) base = atomicAdd(A.next, want);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            // (the head overshoots n by at most 64 per wave and round after it ran dry, once: `dry` stops further fetches)
            if (base >= A.n || A.n - base < want) dry = true;
            if (!have && base < A.n && prefix < A.n - base) {
                mine = base + prefix;
                s = A.shadow[mine]; c = A.closest[mine];
                have = true;
            }
        }
        if (__ballot(have) == 0ull) break;
        if (round >= A.round_cap) {
            if (have) { Hit none; none.prim = 0xffffffffu; trace_store(A.out, mine, false, none, HJR_TRACE_STATUS_ROUND_CAP); }
            break;
        }
        Counters ca, cb; ca.box = ca.tri = cb.box = cb.tri = 0;
        const bool a_valid = have && s.valid != 0u, b_valid = have && c.valid != 0u;
        inflight = traverse_fused<false, WIDTH, BLOCK, typename L::ST, (LDSBVH ? HJR_CARRY_LDS : HJR_CARRY_MEM)>(
            nodes, tris, a_valid, V(s.o[0], s.o[1], s.o[2]), V(s.d[0], s.d[1], s.d[2]), s.tmax, b_valid, V(c.o[0], c.o[1], c.o[2]), V(c.d[0], c.d[1], c.d[2]),
            occluded, h, stack, ca, cb, inflight, tc, A.P.node_min);
        if (have && !inflight) {
            trace_store(A.out, mine, occluded, h, HJR_TRACE_STATUS_OK);
            have = false;
        }
    }
    L::flush_overflow(stack, A.n_over);
}

// hjr_util.hip::hjr_trace_rays calls these; each is launch_trace_batch of its unit
int hjr_launch_trace(hjr_ctx* c, const LaunchPlan& pl, bool fused, const TraceArgs& a, hipStream_t st);      // hjr_launch_trace.hip
int hjr_launch_trace_fast(hjr_ctx* c, const LaunchPlan& pl, bool fused, const TraceArgs& a, hipStream_t st); // hjr_launch_fast_trace.hip

#ifdef HJR_TRACE_UNIT /* the two translation units that hold the kernels */
using TraceKernel = void (*)(TraceArgs);
template <bool FUSED, int BLOCK, bool LDSBVH, bool STACK16, int WIDTH> static TraceKernel trace_kernel_of()
{
    if (FUSED) return hjr_trace_fused_kernel<BLOCK, LDSBVH, STACK16, WIDTH, HJR_FAST_TAG>;
    return hjr_trace_standalone_kernel<BLOCK, LDSBVH, STACK16, WIDTH, HJR_FAST_TAG>;
}
template <bool FUSED> static TraceKernel pick_trace_kernel(int lds_mode)
{
    switch (lds_mode) {
    case 0: return trace_kernel_of<FUSED, HJR_BLOCK, false, false, 4>();
    case 1: return trace_kernel_of<FUSED, HJR_BLOCK_LDS, true, false, 2>();
    case 2: return trace_kernel_of<FUSED, HJR_BLOCK_LDS, true, true, 2>();
    case 3: return trace_kernel_of<FUSED, HJR_BLOCK, false, false, 2>();
    }
    return nullptr;
}

// The launch of one batch with the kernels of THIS translation unit: a small persistent grid (one workgroup for the LDS layouts, two for the
// memory layouts), the dynamic-LDS limit, and the overflow buffer of the short stacks sized as launch_plan sizes it.
// hjr_launch_trace (exact flags) and hjr_launch_trace_fast (FASTFLAGS) are this function in the two units.
static int launch_trace_batch(hjr_ctx* c, const LaunchPlan& pl, bool fused, TraceArgs a, hipStream_t st)
{
    const TraceKernel kern = fused ? pick_trace_kernel<true>(pl.lds_mode) : pick_trace_kernel<false>(pl.lds_mode);
    if (!kern) { set_error("hjr_trace_rays: no kernel for lds_mode " + std::to_string(pl.lds_mode)); return HJR_ERR_DEVICE; }
    const bool lds_layout = pl.lds_mode == 1 || pl.lds_mode == 2;
    const unsigned blocks = lds_layout ? 1u : 2u;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.smem) != hipSuccess) {
        set_error("hjr_trace_rays: could not reserve " + std::to_string(pl.smem) + " bytes of dynamic LDS");
        return HJR_ERR_DEVICE;
    }
    a.P = pl.kp;
    if (pl.spill_buf) {
        a.P.spill_stride = blocks * pl.block;
        const uint32_t over = a.P.stack_depth > a.P.stack_lds_entries ? a.P.stack_depth - a.P.stack_lds_entries : 0u;
        if (!c->d_spill.reserve((size_t)a.P.spill_stride * (over ? over : 1u) * 4)) { set_error("hjr_trace_rays: stack spill allocation failed"); return HJR_ERR_DEVICE; }
        a.P.stack_spill = (uint32_t*)c->d_spill.p;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(pl.block), pl.smem, st, a);
    return HJR_OK;
}
#endif
