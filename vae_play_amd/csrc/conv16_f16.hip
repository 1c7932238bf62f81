// fp16-pair ("f16") entry points of the split-operand convolution families: their own translation unit, so that the fp16 problem
// descriptors (modes 1 and 2 of igemm16.h) are instantiated here and compile in parallel with conv16.hip's bf16 ones.
#define VP_PCFG_LIBRARY 1
#include "conv16_impl.h"

// checks `products` and hands it to f as a compile-time constant (std::integral_constant<int, 1 | 2 | 3>).  MIN = 1: the entry points that
// have the one-product form (gather, scatter); MIN = 2: the statistics epilogue, which exists for the training arithmetics only.
template <int MIN, class F>
static int with_products(const char* what, int products, F f) {
  VP_REQUIRE(products >= MIN && products <= 3, "%s: products must be %s", what, MIN == 1 ? "1, 2 or 3" : "2 or 3");
  if constexpr (MIN == 1) if (products == 1) return f(std::integral_constant<int, 1>());
  return products == 2 ? f(std::integral_constant<int, 2>()) : f(std::integral_constant<int, 3>());
}
#define VP_PRODUCTS_FROM(MIN, what, call) with_products<MIN>(what, products, [&](auto pr) { constexpr int PR = decltype(pr)::value; return call; })
#define VP_PRODUCTS(what, call) VP_PRODUCTS_FROM(1, what, call)
#define VP_PRODUCTS23(what, call) VP_PRODUCTS_FROM(2, what, call)

extern "C" {

// ---- fp16-pair planes ("f16x2" plans): the same three families with two or three MFMAs per fragment pair (igemm16.h mfma_split) -------
// Operands are written by the *_fmt producers with format 1; `products` = 3: al*bh + ah*bl + ah*bh (forward layers: ~1e-6 relative),
// 1: ah*bh (inference: neither lo plane is read; 11 significant bits per operand),
// 2: (ah + al)*bh (backward layers: the weight operand of the gather / scatter families and the `big` operand of the weight gradient
// contribute their fp16 hi plane only, ~2e-4 relative per layer).  out_scale multiplies the accumulators (1 / the scale the producer
// of a gradient operand applied; 1 for activations and weights).
int vp_conv5_gather_f16(const void* big_split, const void* w_p0_split, const float* bias, float* small_out, int B, int Hs,
                        int Ws, int Cbig, int Csmall, int stride, int act, int products, float out_scale, vp_stream stream) {
  return VP_PRODUCTS("vp_conv5_gather_f16", gather16<PR>("vp_conv5_gather_f16", big_split, w_p0_split, bias, small_out, B, Hs, Ws, Hs * stride,
                                                         Ws * stride, Cbig, Csmall, 5, stride, act, stream, out_scale));
}
int vp_conv_gather_f16(const void* big_split, const void* w_p0_split, const float* bias, float* small_out, int B, int Hs, int Ws,
                       int Hb, int Wb, int Cbig, int Csmall, int ks, int stride, int act, int products, float out_scale, vp_stream stream) {
  return VP_PRODUCTS("vp_conv_gather_f16", gather16<PR>("vp_conv_gather_f16", big_split, w_p0_split, bias, small_out, B, Hs, Ws, Hb, Wb, Cbig,
                                                        Csmall, ks, stride, act, stream, out_scale));
}
int vp_conv5_scatter_f16(const void* small_split, const void* w_p1_split, float* big_out, int B, int Hs, int Ws, int Csmall,
                         int Cbig, int stride, int products, float out_scale, vp_stream stream) {
  return VP_PRODUCTS("vp_conv5_scatter_f16", scatter16<PR>("vp_conv5_scatter_f16", small_split, w_p1_split, big_out, B, Hs, Ws, Hs * stride,
                                                           Ws * stride, Csmall, Cbig, 5, stride, stream, out_scale));
}
int vp_conv_scatter_f16(const void* small_split, const void* w_p1_split, float* big_out, int B, int Hs, int Ws, int Hb, int Wb,
                        int Csmall, int Cbig, int ks, int stride, int products, float out_scale, vp_stream stream) {
  return VP_PRODUCTS("vp_conv_scatter_f16", scatter16<PR>("vp_conv_scatter_f16", small_split, w_p1_split, big_out, B, Hs, Ws, Hb, Wb, Csmall,
                                                          Cbig, ks, stride, stream, out_scale));
}
int vp_conv5_wgrad_f16x2(const void* big_split, const void* small_split, float* dw_ref, int B, int Hs, int Ws, int Cbig,
                         int Csmall, int stride, float out_scale, void* ws, size_t ws_bytes, vp_stream stream) {
  return wgrad16<2>("vp_conv5_wgrad_f16x2", big_split, small_split, dw_ref, B, Hs, Ws, Hs * stride, Ws * stride, Cbig, Csmall, 5, stride, ws,
                    ws_bytes, stream, out_scale);
}
int vp_conv5_wgrad_f16x2_cus(const void* big_split, const void* small_split, float* dw_ref, int B, int Hs, int Ws, int Cbig,
                             int Csmall, int stride, float out_scale, int max_cus, void* ws, size_t ws_bytes, vp_stream stream) {
  return wgrad16<2>("vp_conv5_wgrad_f16x2_cus", big_split, small_split, dw_ref, B, Hs, Ws, Hs * stride, Ws * stride, Cbig, Csmall, 5, stride, ws,
                    ws_bytes, stream, out_scale, max_cus);
}

int vp_conv_wgrad_f16x2(const void* big_split, const void* small_split, float* dw_ref, int B, int Hs, int Ws, int Hb, int Wb, int Cbig,
                        int Csmall, int ks, int stride, float out_scale, void* ws, size_t ws_bytes, vp_stream stream) {
  return wgrad16<2>("vp_conv_wgrad_f16x2", big_split, small_split, dw_ref, B, Hs, Ws, Hb, Wb, Cbig, Csmall, ks, stride, ws, ws_bytes, stream,
                    out_scale);
}

// BatchNorm statistics from the epilogue on fp16-pair planes (forward layers: out_scale is 1); descriptor mode = products - 1
size_t vp_conv5_stats_f16_workspace_bytes(int family, int B, int Hs, int Ws, int Cbig, int Csmall, int stride) {
  return plan_stats(family, F16_2, B, Hs, Ws, Cbig, Csmall, stride, true, plan_switches()).stat_floats * sizeof(float);
}

int vp_conv5_gather_stats_f16(const void* big_split, const void* w_p0_split, float* small_out, int B, int Hs, int Ws, int Cbig,
                              int Csmall, int stride, int products, float eps, float momentum, float* mean, float* rstd, float* running_mean,
                              float* running_var, void* ws, size_t ws_bytes, vp_stream stream) {
  return VP_PRODUCTS23("vp_conv5_gather_stats_f16",
                     conv5_stats("vp_conv5_gather_stats_f16", "vp_conv5_stats_f16_workspace_bytes", conv_gather<ProbF16T<true, PR - 1>, FORMS_ALL, TILES_ALL>,
                                 0, arith16<PR>(), true, big_split, w_p0_split, small_out, B, Hs, Ws, Cbig, Csmall, stride,
                                 {eps, momentum, mean, rstd, running_mean, running_var, ws, ws_bytes}, stream));
}

int vp_conv5_scatter_stats_f16(const void* small_split, const void* w_p1_split, float* big_out, int B, int Hs, int Ws, int Csmall,
                               int Cbig, int stride, int products, float eps, float momentum, float* mean, float* rstd, float* running_mean,
                               float* running_var, void* ws, size_t ws_bytes, vp_stream stream) {
  return VP_PRODUCTS23("vp_conv5_scatter_stats_f16",
                     conv5_stats("vp_conv5_scatter_stats_f16", "vp_conv5_stats_f16_workspace_bytes", conv_scatter<ProbT16T<true, PR - 1>, FORMS_ALL, TILES_ALL>,
                                 1, arith16<PR>(), true, small_split, w_p1_split, big_out, B, Hs, Ws, Cbig, Csmall, stride,
                                 {eps, momentum, mean, rstd, running_mean, running_var, ws, ws_bytes}, stream));
}

}
