// Kernels of the ray-batch test hook (hjr_trace_rays), exact flags: every layout, the stand-alone and the fused loop.
#define HJR_TRACE_UNIT
#include "hjr_trace_hook.hip.h"
int hjr_launch_trace(hjr_ctx* c, const LaunchPlan& pl, bool fused, const TraceArgs& a, hipStream_t st) { return launch_trace_batch(c, pl, fused, a, st); }
