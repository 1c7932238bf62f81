// Inference: the plain 5x5 gather / scatter convolutions with the eval-mode BatchNorm (+ ReLU) folded into their epilogue
// (igemm16.h ProbAff / epilogue_affine32), in split-bf16, in one-product fp16 and in exact fp32, and the kernel that folds a BatchNorm's running
// statistics into the per-channel scale / shift they take.
//
// Launch shapes are those of the un-fused entry points' igemm16_kernel path (the same planner: launch_plan.h, EPI_AFFINE), minus
// everything that cannot carry the epilogue: K is never split (a non-linear epilogue cannot be applied to partial sums -- shapes
// whose plain launch splits K are reported as unsupported and keep convolution + one normalise pass), and only the 32x32 MFMA form on
// 64-deep channel chunks is instantiated (three tiles per family and arithmetic).
#define VP_PCFG_LIBRARY 1
#include "conv_exec.h"

namespace vp {

// s = gamma / sqrt(var + eps), t = beta - mean * s, rstd = 1 / sqrt(var + eps): formed in fp64 and rounded ONCE to fp32
__global__ void bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ rm,
                               const float* __restrict__ rv, float eps, float* __restrict__ scale, float* __restrict__ shift,
                               float* __restrict__ rstd, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double r = 1.0 / sqrt((double)rv[c] + (double)eps);
  const double s = (gamma ? (double)gamma[c] : 1.0) * r;
  if (scale) scale[c] = (float)s;
  if (shift) shift[c] = (float)((beta ? (double)beta[c] : 0.0) - (double)rm[c] * s);
  if (rstd) rstd[c] = (float)r;
}

// Executes plan_affine's ConvPlan (launch_plan.h) on the family's launcher: the un-fused entry points' staged tile, K order and XCD map.
template <int MODE, bool SCATTER>      // 0: bf16 pairs | 3: fp32 | 4: fp16 hi planes, one product (out_fmt: igemm16.h AffineEpi)
static int conv_affine(const char* what, const void* a, const void* w, const float* scale, const float* shift, float* out, void* out_split, int B,
                       int Hs, int Ws, int Cbig, int Csmall, int stride, int act, vp_stream stream, int out_fmt = 0) {
  const ConvPlan pl = plan_affine(SCATTER, MODE == 3 ? 1 : (MODE == 4 ? 2 : 0), B, Hs, Ws, Cbig, Csmall, stride, plan_switches());
  if (!pl.affine_ok) return fail(VP_ERR_ARG, "%s: this launch shape does not take the affine epilogue (vp_conv5_affine_supported() == 0)", what);
  const ConvGeom g = make_geom(B, Hs, Ws, Csmall, Cbig, stride, 5);
  ConvEpi e;
  e.act = act; e.scale = scale; e.shift = shift; e.out_split = out_split; e.out_fmt = out_fmt;
  if constexpr (SCATTER) return conv_scatter<ProbAff<ProbT16T<true, MODE>>, K64F, T_SQUARE>(what, pl, g, a, w, out, e, stream);
  else return conv_gather<ProbAff<ProbF16T<true, MODE>>, K64F, T_SQUARE>(what, pl, g, a, w, out, e, stream);
}

}  // namespace vp

using namespace vp;
extern "C" {

int vp_bn_fold_f32(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, float* scale,
                   float* shift, float* rstd, int C, vp_stream stream) {
  VP_REQUIRE(running_mean && running_var && (scale || shift || rstd) && C > 0 && eps >= 0.f, "vp_bn_fold_f32: bad arguments");
  hipLaunchKernelGGL(bn_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, gamma, beta, running_mean, running_var, eps,
                     scale, shift, rstd, C);
  return check_launch("vp_bn_fold_f32");
}

int vp_conv5_affine_supported(int family, int precision, int B, int Hs, int Ws, int Cbig, int Csmall, int stride) {
  return plan_affine(family, precision, B, Hs, Ws, Cbig, Csmall, stride, plan_switches()).affine_ok ? 1 : 0;
}

#define VP_AFFINE_CHECKS(what, a, w)                                                                                      \
  VP_REQUIRE(a && w, what ": null operand");                                                                              \
  VP_REQUIRE(scale && shift, what ": null scale / shift");                                                                \
  VP_REQUIRE(out_f32 || out_split, what ": both outputs are null");                                                       \
  VP_REQUIRE(act == VP_ACT_NONE || act == VP_ACT_RELU, what ": the epilogue supports none|relu");                         \
  VP_REQUIRE(aligned16(a, w, out_f32, out_split), what ": operands and outputs must be 16-byte aligned")

int vp_conv5_gather_affine_bf16x3(const void* big_split, const void* w_p0_split, const float* scale, const float* shift, float* out_f32,
                                  void* out_split, int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int act, vp_stream stream) {
  VP_AFFINE_CHECKS("vp_conv5_gather_affine_bf16x3", big_split, w_p0_split);
  return conv_affine<0, false>("vp_conv5_gather_affine_bf16x3", big_split, w_p0_split, scale, shift, out_f32, out_split, B, Hs, Ws, Cbig,
                               Csmall, stride, act, stream);
}

int vp_conv5_scatter_affine_bf16x3(const void* small_split, const void* w_p1_split, const float* scale, const float* shift, float* out_f32,
                                   void* out_split, int B, int Hs, int Ws, int Csmall, int Cbig, int stride, int act, vp_stream stream) {
  VP_AFFINE_CHECKS("vp_conv5_scatter_affine_bf16x3", small_split, w_p1_split);
  return conv_affine<0, true>("vp_conv5_scatter_affine_bf16x3", small_split, w_p1_split, scale, shift, out_f32, out_split, B, Hs, Ws, Cbig,
                              Csmall, stride, act, stream);
}

int vp_conv5_gather_affine_f32(const float* big, const float* w_p0, const float* scale, const float* shift, float* out_f32, void* out_split,
                               int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int act, vp_stream stream) {
  VP_AFFINE_CHECKS("vp_conv5_gather_affine_f32", big, w_p0);
  VP_REQUIRE(!out_split, "vp_conv5_gather_affine_f32: split planes are written by the bf16x3 entry point only");
  return conv_affine<3, false>("vp_conv5_gather_affine_f32", big, w_p0, scale, shift, out_f32, nullptr, B, Hs, Ws, Cbig, Csmall, stride, act, stream);
}

int vp_conv5_scatter_affine_f32(const float* small, const float* w_p1, const float* scale, const float* shift, float* out_f32, void* out_split,
                                int B, int Hs, int Ws, int Csmall, int Cbig, int stride, int act, vp_stream stream) {
  VP_AFFINE_CHECKS("vp_conv5_scatter_affine_f32", small, w_p1);
  VP_REQUIRE(!out_split, "vp_conv5_scatter_affine_f32: split planes are written by the bf16x3 entry point only");
  return conv_affine<3, true>("vp_conv5_scatter_affine_f32", small, w_p1, scale, shift, out_f32, nullptr, B, Hs, Ws, Cbig, Csmall, stride, act,
                              stream);
}

// One-product fp16 (inference): operands are fp16 planes in format 1 of which only the hi planes are read; out_fmt names what out_split gets
int vp_conv5_gather_affine_f16(const void* big_split, const void* w_p0_split, const float* scale, const float* shift, float* out_f32,
                               void* out_split, int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int act, int out_fmt, vp_stream stream) {
  VP_AFFINE_CHECKS("vp_conv5_gather_affine_f16", big_split, w_p0_split);
  VP_REQUIRE(out_fmt >= 0 && out_fmt <= 2, "vp_conv5_gather_affine_f16: out_fmt must be 0, 1 or 2");
  return conv_affine<4, false>("vp_conv5_gather_affine_f16", big_split, w_p0_split, scale, shift, out_f32, out_split, B, Hs, Ws, Cbig, Csmall,
                               stride, act, stream, out_fmt);
}

int vp_conv5_scatter_affine_f16(const void* small_split, const void* w_p1_split, const float* scale, const float* shift, float* out_f32,
                                void* out_split, int B, int Hs, int Ws, int Csmall, int Cbig, int stride, int act, int out_fmt, vp_stream stream) {
  VP_AFFINE_CHECKS("vp_conv5_scatter_affine_f16", small_split, w_p1_split);
  VP_REQUIRE(out_fmt >= 0 && out_fmt <= 2, "vp_conv5_scatter_affine_f16: out_fmt must be 0, 1 or 2");
  return conv_affine<4, true>("vp_conv5_scatter_affine_f16", small_split, w_p1_split, scale, shift, out_f32, out_split, B, Hs, Ws, Cbig, Csmall,
                              stride, act, stream, out_fmt);
}

}
