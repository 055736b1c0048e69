// Render kernels of the MIS integrator (every layout, variant and both kernel families; with and without the statistics counters).
#include "hjr_launch.hip.h"
template int hjr_launch<HJR_INTEGRATOR_MIS, false>(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
template int hjr_launch<HJR_INTEGRATOR_MIS, true>(hjr_ctx*, const LaunchPlan&, uint64_t, hipStream_t);
