// Inference: the plain 5x5 gather / scatter convolutions with the eval-mode BatchNorm (+ ReLU) folded into their epilogue
// (igemm16.h ProbAff / epilogue_affine32), in split-bf16 and in exact fp32, and the kernel that folds a BatchNorm's running
// statistics into the per-channel scale / shift they take.
//
// Launch shapes are those of the un-fused entry points' igemm16_kernel path (same tile rule, same K order, same XCD map), minus
// everything that cannot carry the epilogue: K is never split (a non-linear epilogue cannot be applied to partial sums -- shapes
// whose plain launch splits K are reported as unsupported and keep convolution + one normalise pass), and only the 32x32 MFMA form on
// 64-deep channel chunks is instantiated (three tiles per family and arithmetic).
#define VP_PCFG_LIBRARY 1
#include "conv16_impl.h"
#include "conv32.h"

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
static void launch_affine(const P& p, long M, long N, int gz, hipStream_t s, int bm, int bn) {
  const dim3 block(256);
  auto grid = [&](int tm, int tn) { return dim3((unsigned)((M + tm - 1) / tm), (unsigned)((N + tn - 1) / tn), (unsigned)gz); };
  if (bm == 128 && bn == 128) hipLaunchKernelGGL((igemm16_kernel<P, 128, 128, 2, 2, 64, true>), grid(128, 128), block, 0, s, p);
  else if (bm == 128 && bn == 64) hipLaunchKernelGGL((igemm16_kernel<P, 128, 64, 2, 2, 64, true>), grid(128, 64), block, 0, s, p);
  else hipLaunchKernelGGL((igemm16_kernel<P, 64, 64, 2, 2, 64, true>), grid(64, 64), block, 0, s, p);
}

// precision: 0 = split-bf16, 1 = exact fp32.  Cin = the contracted side's channel count, Cout = the output's.
struct AffPlan { int ok, bm, bn, gz; long M; };
static AffPlan affine_plan(int family, int precision, int B, int Hs, int Ws, int Cbig, int Csmall, int stride) {
  AffPlan a = {0, 0, 0, 0, 0};
  if ((family != 0 && family != 1) || (precision != 0 && precision != 1)) return a;
  if (B <= 0 || Hs <= 0 || Ws <= 0 || Cbig <= 0 || Csmall <= 0 || (stride != 1 && stride != 2)) return a;
  const int Cin = family == 0 ? Cbig : Csmall, Cout = family == 0 ? Csmall : Cbig;
  const int ph = family == 0 ? 1 : stride * stride;
  a.M = (long)B * Hs * Ws;
  a.gz = ph;
  if (Cout < 64 || Cout % 8 != 0) return a;
  const size_t n_in = (size_t)a.M * (family == 0 ? stride * stride : 1) * Cin, n_w = (size_t)Cin * 25 * Cout;
  if (precision == 0) {
    if (Cin % 64 != 0) return a;                                        // 64-deep channel chunks of bf16 pairs
    if ((family == 0 ? gather_nsplit(a.M, Cout, 25 * Cin, Cin, true, false, VP_ACT_NONE) : scatter_nsplit(a.M, Cout, Cin, stride, true)) != 1)
      return a;
    const Tile16 t = choose_tile16(a.M, Cout, ph, false, Cin);
    a.bm = t.bm; a.bn = t.bn;
  } else {
    if (Cin % 32 != 0 || !f32_fast_enabled()) return a;                 // 64-deep chunks of 16-bit units = 32 floats
    if (n_in * 2 >= ((size_t)1 << 31) || n_w * 2 >= ((size_t)1 << 31)) return a;
    if ((family == 0 ? f32_fast_gather_nsplit(a.M, Cout, Cin) : f32_fast_scatter_nsplit(a.M, Cout, Cin, ph)) != 1) return a;
    f32_fast_tile(a.M, Cout, ph, &a.bm, &a.bn);
  }
  if (a.bn == 32) return a;
  a.ok = 1;
  return a;
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

template <int MODE>      // 0: bf16 pairs | 3: fp32
static int gather_affine(const char* what, const void* big, const void* w_p0, const float* scale, const float* shift, float* out, void* out_split,
                         int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int act, vp_stream stream) {
  const AffPlan a = affine_plan(0, MODE == 3 ? 1 : 0, B, Hs, Ws, Cbig, Csmall, stride);
  if (!a.ok) return fail(VP_ERR_ARG, "%s: this launch shape does not take the affine epilogue (vp_conv5_affine_supported() == 0)", what);
  ProbAff<ProbF16T<true, MODE>> p;
  const int C = MODE == 3 ? 2 * Cbig : Cbig;      // gathered channels in 16-bit units
  p.g = make_geom(B, Hs, Ws, Csmall, C, stride, 5, Hs * stride, Ws * stride);
  p.big = (const u16*)big; p.big_plane = MODE == 3 ? 0 : (size_t)B * p.g.Hb * p.g.Wb * Cbig;
  p.w = (const u16*)w_p0; p.w_plane = MODE == 3 ? 0 : (size_t)Csmall * Cbig * 25;
  p.bias = nullptr; p.act = VP_ACT_NONE;
  p.M = (int)a.M; p.N = Csmall; p.K = 25 * C;
  p.k_per_split = p.K;
  fill_epilogue(p, scale, shift, out, out_split, (size_t)a.M * Csmall, act);
  p.xcd_map = xcd_map_tile(p.M, p.N, a.bm, a.bn);
  launch_affine(p, p.M, p.N, 1, (hipStream_t)stream, a.bm, a.bn);
  return check_launch(what);
}

template <int MODE>
static int scatter_affine(const char* what, const void* small, const void* w_p1, const float* scale, const float* shift, float* out,
                          void* out_split, int B, int Hs, int Ws, int Csmall, int Cbig, int stride, int act, vp_stream stream) {
  const AffPlan a = affine_plan(1, MODE == 3 ? 1 : 0, B, Hs, Ws, Cbig, Csmall, stride);
  if (!a.ok) return fail(VP_ERR_ARG, "%s: this launch shape does not take the affine epilogue (vp_conv5_affine_supported() == 0)", what);
  ProbAff<ProbT16T<true, MODE>> p;
  const int C = MODE == 3 ? 2 * Csmall : Csmall;
  p.g = make_geom(B, Hs, Ws, C, Cbig, stride, 5, Hs * stride, Ws * stride);
  p.small = (const u16*)small; p.small_plane = MODE == 3 ? 0 : (size_t)a.M * Csmall;
  p.w = (const u16*)w_p1; p.w_plane = MODE == 3 ? 0 : (size_t)Csmall * Cbig * 25;
  p.M = (int)a.M; p.N = Cbig;
  fill_epilogue(p, scale, shift, out, out_split, (size_t)a.M * stride * stride * Cbig, act);
  p.xcd_map = xcd_map_tile(p.M, p.N, a.bm, a.bn);
  const long wgs = ((a.M + a.bm - 1) / a.bm) * ((p.N + a.bn - 1) / a.bn) * a.gz;
  p.pair_phases = (stride == 2 && wgs <= 512) ? 1 : 0;
  launch_affine(p, p.M, p.N, a.gz, (hipStream_t)stream, a.bm, a.bn);
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
  return affine_plan(family, precision, B, Hs, Ws, Cbig, Csmall, stride).ok;
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
