// Exact-fp32 gather / scatter convolutions of the plain 5x5 layers on the split-operand kernel's data path (round 3).
//
// igemm.h (round 1) decomposes k -> (tap, channel) per 16-B load, predicates, walks K tap-major and never splits K: 41-70 % of the
// fp32-MFMA peak per layer (profiles/r03_*_f32).  igemm16_kernel already has what the 16-bit modes needed -- workgroup-uniform tap
// decomposition, the zero page, channel-chunk-major K order, XCD-aware tile order, 2-way split-K for the few-tile layers -- and its
// data path does not care what the 16-B chunks hold: MODE 3 (igemm16.h) stages ONE plane per operand, reads a fragment as 4 fp32 and
// contracts it with four v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate: the reference's arithmetic,
// models/networks.py:14,38).  The fp32 tensors are addressed in 16-bit units: [pixel][C] fp32 = [pixel][2C] u16, a 64-deep K-tile =
// 32 floats, so the gathered channel count is doubled in the geometry and nothing else changes.
#include "conv_exec.h"
#include "conv32.h"

namespace vp {

typedef ProbF16T<true, 3> ProbF32;      // plain 5x5 only; K-tiles of 64 or 32 u16 without channel tails, the square tiles
typedef ProbT16T<true, 3> ProbT32;
constexpr unsigned FORMS_F32 = K64F | K32F, TILES_F32 = T_SQUARE;

int f32_fast_gather(const char* what, const ConvPlan& pl, const float* big, const float* w_p0, const float* bias, float* out, const ConvGeom& g,
                    int act, vp_stream stream) {
  ConvEpi e;
  e.bias = bias; e.act = act;
  return conv_gather<ProbF32, FORMS_F32, TILES_F32>(what, pl, g, big, w_p0, out, e, stream);
}

int f32_fast_scatter(const char* what, const ConvPlan& pl, const float* small, const float* w_p1, float* out, const ConvGeom& g, vp_stream stream) {
  return conv_scatter<ProbT32, FORMS_F32, TILES_F32>(what, pl, g, small, w_p1, out, ConvEpi(), stream);
}

}  // namespace vp

using namespace vp;
extern "C" {

// BatchNorm statistics from the epilogue (as vp_conv5_*_stats_bf16x3): {pivot, sum(x - pivot), sum((x - pivot)^2)} per (workgroup, channel)
// straight from the fp32 accumulators + one finaliser launch; removes bn_partial_kernel<0>'s read of the activation for the layers that
// do not split K
size_t vp_conv5_stats_f32_workspace_bytes(int family, int B, int Hs, int Ws, int Cbig, int Csmall, int stride) {
  return plan_stats(family, F32, B, Hs, Ws, Cbig, Csmall, stride, true, plan_switches()).stat_floats * sizeof(float);
}

int vp_conv5_gather_stats_f32(const float* big, const float* w_p0, float* small_out, int B, int Hs, int Ws, int Cbig, int Csmall, int stride,
                              float eps, float momentum, float* mean, float* rstd, float* running_mean, float* running_var, void* ws,
                              size_t ws_bytes, vp_stream stream) {
  return conv5_stats("vp_conv5_gather_stats_f32", "vp_conv5_stats_f32_workspace_bytes", conv_gather<ProbF32, FORMS_F32, TILES_F32>, 0, F32,
                     aligned16(big, w_p0), big, w_p0, small_out, B, Hs, Ws, Cbig, Csmall, stride,
                     {eps, momentum, mean, rstd, running_mean, running_var, ws, ws_bytes}, stream);
}

int vp_conv5_scatter_stats_f32(const float* small, const float* w_p1, float* big_out, int B, int Hs, int Ws, int Csmall, int Cbig, int stride,
                               float eps, float momentum, float* mean, float* rstd, float* running_mean, float* running_var, void* ws,
                               size_t ws_bytes, vp_stream stream) {
  return conv5_stats("vp_conv5_scatter_stats_f32", "vp_conv5_stats_f32_workspace_bytes", conv_scatter<ProbT32, FORMS_F32, TILES_F32>, 1, F32,
                     aligned16(small, w_p1), small, w_p1, big_out, B, Hs, Ws, Cbig, Csmall, stride,
                     {eps, momentum, mean, rstd, running_mean, running_var, ws, ws_bytes}, stream);
}

}
