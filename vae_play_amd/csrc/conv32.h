// fp32 gather / scatter on the split-operand kernel's data path (conv32.hip)
#pragma once
#include <hip/hip_runtime.h>
#include "launch_plan.h"
namespace vp {
// execute a plan_conv(.., F32, ..) plan whose route is ROUTE_STAGED; `stat`: per-workgroup BatchNorm statistics slab of the epilogue
// (igemm16.h epilogue_stats32), or nullptr
int f32_fast_gather(const ConvPlan& pl, const float* big, const float* w_p0, const float* bias, float* out, const ConvGeom& g, int act, hipStream_t s,
                    float* stat = nullptr);
int f32_fast_scatter(const ConvPlan& pl, const float* small, const float* w_p1, float* out, const ConvGeom& g, hipStream_t s, float* stat = nullptr);
// finaliser of the epilogue statistics for every arithmetic (conv16.hip): the slab geometry is the launch's plan
int stats_finish(const ConvPlan& pl, const float* slab, float eps, float momentum, float* mean, float* rstd, float* rm, float* rv, hipStream_t stream,
                 const char* what);
}
