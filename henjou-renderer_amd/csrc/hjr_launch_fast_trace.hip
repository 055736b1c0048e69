// The same kernels of the ray-batch test hook compiled like the approximate-arithmetic render kernels (Makefile: FASTFLAGS): HJR_TRACE_FAST_BUILD.
// The traversal and the triangle test must be the same operations here (hjr_traverse.hip.h); tests/test_gpu_trace.py compares the two builds bit for bit.
#ifndef HJR_FAST_MATH
#error "compile this unit with -DHJR_FAST_MATH (Makefile: build/hjr_launch_fast_%.o)"
#endif
#define HJR_TRACE_UNIT
#include "hjr_trace_hook.hip.h"
int hjr_launch_trace_fast(hjr_ctx* c, const LaunchPlan& pl, bool fused, const TraceArgs& a, hipStream_t st) { return launch_trace_batch(c, pl, fused, a, st); }
