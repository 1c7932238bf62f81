// Inference: the plain 5x5 gather / scatter convolutions with the eval-mode BatchNorm (+ ReLU) folded into their epilogue
// (igemm16.h ProbAff / epilogue_affine32), in split-bf16 and in exact fp32, and the kernel that folds a BatchNorm's running
// statistics into the per-channel scale / shift they take.
//
// Launch shapes are those of the un-fused entry points' igemm16_kernel path (the same planner: launch_plan.h, EPI_AFFINE), minus
// everything that cannot carry the epilogue: K is never split (a non-linear epilogue cannot be applied to partial sums -- shapes
// whose plain launch splits K are reported as unsupported and keep convolution + one normalise pass), and only the 32x32 MFMA form on
// 64-deep channel chunks is instantiated (three tiles per family and arithmetic).
#define VP_PCFG_LIBRARY 1
#include "conv16_impl.h"

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

template <class P>
static void fill_epilogue(P& p, const float* scale, const float* shift, float* out, void* out_split, size_t n_out, int act) {
  p.alpha = 1.f;
  p.zero = vp_zero_page();
  p.out = out;
  p.nsplit = 1;
  p.stat = nullptr;
  p.e.scale = scale; p.e.shift = shift;
  p.e.out_split = (u16*)out_split; p.e.split_plane = n_out;
  p.e.relu = act == VP_ACT_RELU ? 1 : 0;
}

// Both launchers execute plan_affine's ConvPlan (launch_plan.h): the un-fused entry points' staged tile, K order and XCD map.
template <int MODE>      // 0: bf16 pairs | 3: fp32
static int gather_affine(const char* what, const void* big, const void* w_p0, const float* scale, const float* shift, float* out, void* out_split,
                         int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int act, vp_stream stream) {
  const ConvPlan a = plan_affine(0, MODE == 3 ? 1 : 0, B, Hs, Ws, Cbig, Csmall, stride, plan_switches());
  if (!a.affine_ok) return fail(VP_ERR_ARG, "%s: this launch shape does not take the affine epilogue (vp_conv5_affine_supported() == 0)", what);
  ProbAff<ProbF16T<true, MODE>> p;
  const int C = MODE == 3 ? 2 * Cbig : Cbig;      // gathered channels in 16-bit units
  p.g = make_geom(B, Hs, Ws, Csmall, C, stride, 5, Hs * stride, Ws * stride);
  p.big = (const u16*)big; p.big_plane = MODE == 3 ? 0 : (size_t)B * p.g.Hb * p.g.Wb * Cbig;
  p.w = (const u16*)w_p0; p.w_plane = MODE == 3 ? 0 : (size_t)Csmall * Cbig * 25;
  p.bias = nullptr; p.act = VP_ACT_NONE;
  p.M = (int)a.M; p.N = Csmall; p.K = (int)a.K;
  p.k_per_split = a.k_per_split;
  fill_epilogue(p, scale, shift, out, out_split, (size_t)a.M * Csmall, act);
  p.xcd_map = a.xcd_map;
  if (!launch_tiles16<decltype(p), K64F, T_SQUARE>(p, a.bm, a.bn, a.bk, a.fast, false, a.M, a.N, a.gz, (hipStream_t)stream))
    return fail(VP_ERR_LAUNCH, "%s: no kernel for the planned %dx%d tile", what, a.bm, a.bn);
  return check_launch(what);
}

template <int MODE>
static int scatter_affine(const char* what, const void* small, const void* w_p1, const float* scale, const float* shift, float* out,
                          void* out_split, int B, int Hs, int Ws, int Csmall, int Cbig, int stride, int act, vp_stream stream) {
  const ConvPlan a = plan_affine(1, MODE == 3 ? 1 : 0, B, Hs, Ws, Cbig, Csmall, stride, plan_switches());
  if (!a.affine_ok) return fail(VP_ERR_ARG, "%s: this launch shape does not take the affine epilogue (vp_conv5_affine_supported() == 0)", what);
  ProbAff<ProbT16T<true, MODE>> p;
  const int C = MODE == 3 ? 2 * Csmall : Csmall;
  p.g = make_geom(B, Hs, Ws, C, Cbig, stride, 5, Hs * stride, Ws * stride);
  p.small = (const u16*)small; p.small_plane = MODE == 3 ? 0 : (size_t)a.M * Csmall;
  p.w = (const u16*)w_p1; p.w_plane = MODE == 3 ? 0 : (size_t)Csmall * Cbig * 25;
  p.M = (int)a.M; p.N = Cbig;
  fill_epilogue(p, scale, shift, out, out_split, (size_t)a.M * stride * stride * Cbig, act);
  p.xcd_map = a.xcd_map;
  p.pair_phases = a.pair_phases;
  if (!launch_tiles16<decltype(p), K64F, T_SQUARE>(p, a.bm, a.bn, a.bk, a.fast, false, a.M, a.N, a.gz, (hipStream_t)stream))
    return fail(VP_ERR_LAUNCH, "%s: no kernel for the planned %dx%d tile", what, a.bm, a.bn);
  return check_launch(what);
}

static bool aligned16(const void* a, const void* b, const void* c, const void* d) {
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
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
  return gather_affine<0>("vp_conv5_gather_affine_bf16x3", big_split, w_p0_split, scale, shift, out_f32, out_split, B, Hs, Ws, Cbig, Csmall,
                          stride, act, stream);
}

int vp_conv5_scatter_affine_bf16x3(const void* small_split, const void* w_p1_split, const float* scale, const float* shift, float* out_f32,
                                   void* out_split, int B, int Hs, int Ws, int Csmall, int Cbig, int stride, int act, vp_stream stream) {
  VP_AFFINE_CHECKS("vp_conv5_scatter_affine_bf16x3", small_split, w_p1_split);
  return scatter_affine<0>("vp_conv5_scatter_affine_bf16x3", small_split, w_p1_split, scale, shift, out_f32, out_split, B, Hs, Ws, Csmall,
                           Cbig, stride, act, stream);
}

int vp_conv5_gather_affine_f32(const float* big, const float* w_p0, const float* scale, const float* shift, float* out_f32, void* out_split,
                               int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int act, vp_stream stream) {
  VP_AFFINE_CHECKS("vp_conv5_gather_affine_f32", big, w_p0);
  VP_REQUIRE(!out_split, "vp_conv5_gather_affine_f32: split planes are written by the bf16x3 entry point only");
  return gather_affine<3>("vp_conv5_gather_affine_f32", big, w_p0, scale, shift, out_f32, nullptr, B, Hs, Ws, Cbig, Csmall, stride, act, stream);
}

int vp_conv5_scatter_affine_f32(const float* small, const float* w_p1, const float* scale, const float* shift, float* out_f32, void* out_split,
                                int B, int Hs, int Ws, int Csmall, int Cbig, int stride, int act, vp_stream stream) {
  VP_AFFINE_CHECKS("vp_conv5_scatter_affine_f32", small, w_p1);
  VP_REQUIRE(!out_split, "vp_conv5_scatter_affine_f32: split planes are written by the bf16x3 entry point only");
  return scatter_affine<3>("vp_conv5_scatter_affine_f32", small, w_p1, scale, shift, out_f32, nullptr, B, Hs, Ws, Csmall, Cbig, stride, act,
                           stream);
}

}
