// fp32 gather / scatter on the split-operand kernel's data path (conv32.hip), for conv.hip, which does not see igemm16.h
#pragma once
#include "common.h"
namespace vp {
// execute a plan_conv(.., F32, ..) plan whose route is ROUTE_STAGED; `what`: the entry point that was called
int f32_fast_gather(const char* what, const ConvPlan& pl, const float* big, const float* w_p0, const float* bias, float* out, const ConvGeom& g,
                    int act, vp_stream stream);
int f32_fast_scatter(const char* what, const ConvPlan& pl, const float* small, const float* w_p1, float* out, const ConvGeom& g, vp_stream stream);
}
