// Host-side dispatch hooks of halo.hip (halo-resident MFMA convolution for narrow channel counts).
#pragma once
#include <hip/hip_runtime.h>

namespace vp {
// kind: halo_gather_kind / halo_scatter_kind (launch_plan.h), never 0
int halo_gather_launch(int kind, const void* big_split, const void* w_p0_split, const float* bias, float* out, int B, int Hs, int Ws,
                       int Cbig, int Csmall, int stride, int act, hipStream_t s);
int halo_scatter_launch(int kind, const void* small_split, const void* w_p1_split, float* big_out, int B, int Hs, int Ws, int Csmall,
                        int Cbig, hipStream_t s);
}  // namespace vp
