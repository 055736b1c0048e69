// The launch code of the two render-kernel families: hjr_render.hip::plan_launch decides a launch (a LaunchPlan, hjr_context.h), and
// hjr_launch<I, STATS> / hjr_launch_fast<I> turn the plan into a kernel of their translation unit and launch it.  They are instantiated per
// integrator in hjr_launch_{nee,pt,mis}.hip / hjr_launch_fast_*.hip, so that the units compile in parallel; hjr_render.hip only declares them.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <type_traits>

#include "hjr_context.h"
#include "hjr_kernel.hip.h"
#include "hjr_wavefront.hip.h"

#ifdef HJR_FAST_MATH
#define HJR_FAST_TAG true
#else
#define HJR_FAST_TAG false
#endif
using RenderKernel = void (*)(KParams);

template <class F> static RenderKernel with_variant(int var, F f)
{
    return var == 2 ? f(std::integral_constant<int, 2>()) : var == 1 ? f(std::integral_constant<int, 1>()) : f(std::integral_constant<int, 0>());
}
template <int I, bool S, bool LDS, int W, int A, bool WIN = false> static RenderKernel wf_kernel(bool spill)
{
    return spill ? hjr_wavefront_kernel<I, S, HJR_BLOCK_LDS, LDS, true, W, A, WIN> : hjr_wavefront_kernel<I, S, HJR_BLOCK_LDS, LDS, false, W, A, WIN>;
}
// the wavefront kernel of the plan's layout (stack entries are always 32-bit here); window launches make the same choice among the WIN instantiations
template <int I, bool S, int A, bool WIN> static RenderKernel wf_layout_kernel(const LaunchPlan& pl)
{
    if (pl.lds_mode == 1 || pl.lds_mode == 2) return wf_kernel<I, S, true, 2, A, WIN>(pl.wf_spill);
    if (pl.lds_mode == 3) return wf_kernel<I, S, false, 2, A, WIN>(pl.wf_spill);
    return wf_kernel<I, S, false, 4, A, WIN>(pl.wf_spill);
}
template <int I, bool S, int A, bool SINGLE, bool WIN = false> static RenderKernel mega_kernel(int lds_mode)
{
    if (lds_mode == 1) return hjr_render_kernel<I, S, HJR_BLOCK_LDS, true, false, 2, A, HJR_FAST_TAG, SINGLE, WIN>;
    if (lds_mode == 0) return hjr_render_kernel<I, S, HJR_BLOCK, false, false, 4, A, HJR_FAST_TAG, SINGLE, WIN>;
#ifndef HJR_LEAN_VARIANT
    if (lds_mode == 2) return hjr_render_kernel<I, S, HJR_BLOCK_LDS, true, true, 2, A, HJR_FAST_TAG, SINGLE, WIN>;
    if (lds_mode == 3) return hjr_render_kernel<I, S, HJR_BLOCK, false, false, 2, A, HJR_FAST_TAG, SINGLE, WIN>;
#endif
    return nullptr;
}
// the kernels of this translation unit; the lean experiment build has only the NEE non-counting LDS / BVH4-memory megakernels
template <int I, bool S> static RenderKernel pick_kernel(const LaunchPlan& pl)
{
    return with_variant(pl.var, [&](auto var) -> RenderKernel {
        constexpr int A = decltype(var)::value;
#if !defined(HJR_FAST_MATH) && !defined(HJR_LEAN_VARIANT)
        if (pl.wf) return pl.window ? wf_layout_kernel<I, S, A, true>(pl) : wf_layout_kernel<I, S, A, false>(pl);
#endif
#ifndef HJR_LEAN_VARIANT
        // a window launch runs single chunks (hjr_render.hip: launch_render), so the WIN megakernels exist in the SINGLE form only
        if (pl.window) return mega_kernel<I, S, A, true, true>(pl.lds_mode);
#endif
        // items of several chunks (kp.item_chunks > 1; NEE and Pathtrace) run the kernels that carry the item rule, every other launch the
        // SINGLE instantiations, which do not (hjr_kernel.hip.h: close_sample)
        if constexpr (I != HJR_INTEGRATOR_MIS) if (pl.kp.item_chunks > 1u) return mega_kernel<I, S, A, false>(pl.lds_mode);
        return mega_kernel<I, S, A, true>(pl.lds_mode);
    });
}

// Grid, LDS limit, spill and context buffers, launch.  Returns HJR_OK or HJR_ERR_DEVICE (with the failed step in the error text).
static int launch_plan(hjr_ctx* c, const LaunchPlan& pl, RenderKernel kern, uint64_t n_items, hipStream_t st)
{
    if (!kern) { set_error("hjr_render: this build has no kernel for lds_mode " + std::to_string(pl.lds_mode)); return HJR_ERR_DEVICE; }
    // persistent grid = resident workgroups only: CUs x (workgroups the kernel's VGPR/LDS budget admits per CU), capped by the
    // number of batches of work; option "blocks_per_cu" overrides the occupancy query
    int per_cu = pl.per_cu;
    if (per_cu == 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kern, pl.block, pl.smem) != hipSuccess || per_cu < 1)) {
        per_cu = 2;
        (void)hipGetLastError(); // a failed query must not show up as the error of this launch
    }
    uint64_t blocks = (uint64_t)c->n_cus * (uint64_t)per_cu;
    const uint64_t per_block = pl.wf ? pl.kp.wf_cap : pl.block; // work items a workgroup holds at a time
    const uint64_t max_useful = (n_items + per_block - 1) / per_block;
    if (blocks > max_useful) blocks = max_useful ? max_useful : 1;
    if (pl.set_smem && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.smem) != hipSuccess) {
        set_error("hjr_render: could not reserve " + std::to_string(pl.smem) + " bytes of dynamic LDS");
        (void)hipGetLastError(); // the refusal is reported here: the runtime's last-error slot must not fail the context's next launch
        return HJR_ERR_DEVICE;
    }
    KParams kp = pl.kp;
    if (pl.wf) { // context records, then (albedo / normal launches) the AOV sums
        const size_t per_ctx_f4 = HJR_WF_CTX_F4 + (pl.var ? HJR_WF_AOV_F4 : 0);
        if (!c->d_wf_ctx.reserve(per_ctx_f4 * 16 * blocks * kp.wf_cap)) { set_error("hjr_render: wavefront context allocation failed"); return HJR_ERR_DEVICE; }
        kp.wf_ctx = (float4*)c->d_wf_ctx.p;
        kp.wf_aov = pl.var ? kp.wf_ctx + (size_t)HJR_WF_CTX_F4 * blocks * kp.wf_cap : nullptr;
    }
    if (pl.spill_buf) {
        kp.spill_stride = (uint32_t)(blocks * pl.block);
        const uint32_t over = kp.stack_depth > kp.stack_lds_entries ? kp.stack_depth - kp.stack_lds_entries : 0u;
        if (!c->d_spill.reserve((size_t)kp.spill_stride * (over ? over : 1u) * 4)) { set_error("hjr_render: stack spill allocation failed"); return HJR_ERR_DEVICE; }
        kp.stack_spill = (uint32_t*)c->d_spill.p;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(pl.block), pl.smem, st, kp);
    return HJR_OK;
}

#ifdef HJR_FAST_MATH
// HJR_FLAG_FAST_MATH launches: the megakernel family of this (approximate-arithmetic) translation unit, every layout; no counting variant
template <int I> int hjr_launch_fast(hjr_ctx* c, const LaunchPlan& pl, uint64_t n_items, hipStream_t st)
{
    return launch_plan(c, pl, pick_kernel<I, false>(pl), n_items, st);
}
#else
template <int I, bool S> int hjr_launch(hjr_ctx* c, const LaunchPlan& pl, uint64_t n_items, hipStream_t st)
{
    return launch_plan(c, pl, pick_kernel<I, S>(pl), n_items, st);
}
#endif
