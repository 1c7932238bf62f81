// Shared by conv16.hip (bf16 pairs) and conv16_f16.hip (fp16 pairs): argument checks and dispatch of the three split-operand families
// onto the launchers of conv_exec.h (gather, scatter) and the weight-gradient launchers below, which execute the plans of launch_plan.h.
// Everything here is static / a template, so that each translation unit instantiates only the problem descriptors it dispatches (the
// fp16 modes live in their own object file: the two compile in parallel).  `what` names the entry point that was called.
#pragma once
#include "conv_exec.h"
#include "wgrad5.h"
#include "halo.h"
#include "narrow.h"
#include "split.h"

using namespace vp;


template <int F16> constexpr Arith arith16() { return F16 == 0 ? BF16X3 : (F16 == 1 ? F16_1 : (F16 == 2 ? F16_2 : F16_3)); }

// The one-tap-per-workgroup weight gradient on a WgradPlan (WIDE or MAIN): FORMS / TILES name what PW instantiates (igemm16.h)
template <class PW, unsigned FORMS, unsigned TILES>
static int wgrad16_t(const WgradPlan& w, const ConvGeom& g, const void* big_split, const void* small_split, float* dw_ref, void* ws,
                     vp_stream stream, float alpha, const char* what) {
  PW p;
  p.alpha = alpha;
  p.zero = vp_zero_page();
  p.g = g;
  p.big = (const u16*)big_split; p.big_plane = (size_t)g.B * g.Hb * g.Wb * g.Cb;
  p.small = (const u16*)small_split; p.small_plane = (size_t)g.B * g.Hs * g.Ws * g.Cs;
  p.slab = (float*)ws; p.M = g.Cs; p.N = w.N; p.K = g.B * g.Hs * g.Ws;
  p.nsplit = w.nsplit;
  p.k_per_split = w.k_per_split;
  if (!launch_tiles16<PW, FORMS, TILES>(p, w.bm, w.bn, w.bk, w.fast, false, g.Cs, w.N, w.gz, (hipStream_t)stream))
    return fail(VP_ERR_LAUNCH, "%s: no kernel for the planned %dx%d tile", what, w.bm, w.bn);
  int rc = check_launch(what);
  if (rc) return rc;
  return slab_reduce_launch((const float*)ws, dw_ref, g.Cs, g.Cb, w.slabs, (hipStream_t)stream, g.nt);
}

template <int MODE>      // row-of-taps weight gradient (wgrad5.h)
static int wgrad16_rows(const char* what, const WgradPlan& w, const void* big_split, const void* small_split, float* dw_ref, const ConvGeom& g,
                        void* ws, vp_stream stream, float alpha) {
  int slabs = 0;
  wgrad5_launch<MODE>(big_split, small_split, (float*)ws, g, w.kind, w.nsplit, w.k_per_split, alpha, (hipStream_t)stream, &slabs);
  int rc = check_launch(what);
  if (rc) return rc;
  return slab_reduce_launch((const float*)ws, dw_ref, g.Cs, g.Cb, slabs, (hipStream_t)stream, g.nt);
}

// ---- argument checks + dispatch of the three families; F16 = 0: bf16 pairs (three products), 1 | 2 | 3: fp16 planes, products per fragment
// pair (1: hi planes only, descriptor mode 4 -- gather and scatter; the weight gradient has the two-product form only)
template <int F16>
static int gather16(const char* what, const void* big_split, const void* w_p0_split, const float* bias, float* small_out, int B, int Hs,
                    int Ws, int Hb, int Wb, int Cbig, int Csmall, int ks, int stride, int act, vp_stream stream, float alpha = 1.f) {
  VP_REQUIRE(big_split && w_p0_split && small_out, "%s: null pointer", what);
  VP_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Cbig > 0 && Csmall > 0 && Cbig % 8 == 0, "%s: Cbig must be a multiple of 8", what);
  VP_REQUIRE(stride == 1 || stride == 2, "%s: stride must be 1 or 2", what);
  VP_REQUIRE(ks == 1 || ks == 3 || ks == 4 || ks == 5, "%s: kernel size must be 1, 3, 4 or 5", what);
  VP_REQUIRE(act == VP_ACT_NONE || act == VP_ACT_SIGMOID || act == VP_ACT_RELU, "%s: epilogue supports none|sigmoid|relu", what);
  if constexpr (F16 != 0) VP_REQUIRE(alpha > 0.f, "%s: out_scale must be positive", what);
  const ConvGeom g = make_geom(B, Hs, Ws, Csmall, Cbig, stride, ks, Hb, Wb);
  const ConvPlan pl = plan_conv(false, g, arith16<F16>(), bias != nullptr, act, true, EPI_NONE, plan_switches());
  ConvEpi e;
  e.bias = bias; e.act = act; e.alpha = alpha;
#define VP_G16(PF) conv_gather<PF, FORMS_ALL, TILES_ALL>(what, pl, g, big_split, w_p0_split, small_out, e, stream)
  // fp16-pair planes, f16 = products per fragment pair: always the implicit-GEMM kernels (the halo kernels read bf16 pairs)
  if constexpr (F16 == 1) return plain5(g) ? VP_G16(ProbF16O) : VP_G16(ProbF16KO);
  else if constexpr (F16 == 2) return plain5(g) ? VP_G16(ProbF16X) : VP_G16(ProbF16KX);
  else if constexpr (F16 == 3) return plain5(g) ? VP_G16(ProbF16H) : VP_G16(ProbF16KH);
  else {
    if (pl.route == ROUTE_HALO)
      return halo_gather_launch(pl.kind, big_split, w_p0_split, bias, small_out, B, Hs, Ws, Cbig, Csmall, stride, act, (hipStream_t)stream);
    return plain5(g) ? VP_G16(ProbF16) : VP_G16(ProbF16K);
  }
#undef VP_G16
}

template <int F16>
static int scatter16(const char* what, const void* small_split, const void* w_p1_split, float* big_out, int B, int Hs, int Ws, int Hb, int Wb,
                     int Csmall, int Cbig, int ks, int stride, vp_stream stream, float alpha = 1.f, const float* bias = nullptr) {
  VP_REQUIRE(small_split && w_p1_split && big_out, "%s: null pointer", what);
  VP_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Cbig > 0 && Csmall > 0 && Csmall % 8 == 0, "%s: Csmall must be a multiple of 8", what);
  VP_REQUIRE(stride == 1 || stride == 2, "%s: stride must be 1 or 2", what);
  VP_REQUIRE(ks == 1 || ks == 3 || ks == 4 || ks == 5, "%s: kernel size must be 1, 3, 4 or 5", what);
  if constexpr (F16 != 0) VP_REQUIRE(alpha > 0.f, "%s: out_scale must be positive", what);
  const ConvGeom g = make_geom(B, Hs, Ws, Csmall, Cbig, stride, ks, Hb, Wb);
  const ConvPlan pl = plan_conv(true, g, arith16<F16>(), bias != nullptr, VP_ACT_NONE, true, EPI_NONE, plan_switches());
  ConvEpi e;
  e.bias = bias; e.alpha = alpha;
#define VP_S16(PT) conv_scatter<PT, FORMS_ALL, TILES_ALL>(what, pl, g, small_split, w_p1_split, big_out, e, stream)
  if constexpr (F16 == 1) return plain5(g) ? VP_S16(ProbT16O) : VP_S16(ProbT16KO);
  else if constexpr (F16 == 2) return plain5(g) ? VP_S16(ProbT16X) : VP_S16(ProbT16KX);
  else if constexpr (F16 == 3) return plain5(g) ? VP_S16(ProbT16H) : VP_S16(ProbT16KH);
  else {
    if (pl.route == ROUTE_HALO) return halo_scatter_launch(pl.kind, small_split, w_p1_split, big_out, B, Hs, Ws, Csmall, Cbig, (hipStream_t)stream);
    // with a bias (vp_conv_scatter_bias_bf16x3): always the generic-geometry kernel, whose epilogue adds it
    return (plain5(g) && !bias) ? VP_S16(ProbT16) : VP_S16(ProbT16K);
  }
#undef VP_S16
}

template <int F16>
static int wgrad16(const char* what, const void* big_split, const void* small_split, float* dw_ref, int B, int Hs, int Ws, int Hb, int Wb,
                   int Cbig, int Csmall, int ks, int stride, void* ws, size_t ws_bytes, vp_stream stream, float alpha = 1.f, int max_cus = 0) {
  static_assert(F16 == 0 || F16 == 2, "weight gradients have no 3-product fp16 form");
  VP_REQUIRE(big_split && small_split && dw_ref && ws, "%s: null pointer", what);
  VP_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Cbig % 8 == 0 && Csmall % 8 == 0 && Cbig > 0 && Csmall > 0,
             "%s: channel counts must be multiples of 8", what);
  VP_REQUIRE(stride == 1 || stride == 2, "%s: stride must be 1 or 2", what);
  VP_REQUIRE(ks == 1 || ks == 3 || ks == 4 || ks == 5, "%s: kernel size must be 1, 3, 4 or 5", what);
  const ConvGeom g = make_geom(B, Hs, Ws, Csmall, Cbig, stride, ks, Hb, Wb);
  const WgradPlan w = plan_wgrad(g, arith16<F16>(), max_cus, ws_bytes, true, plan_switches());
  if (ws_bytes / sizeof(float) < w.need_floats) return fail(VP_ERR_WORKSPACE, "%s: workspace too small", what);
  if constexpr (F16 != 0) VP_REQUIRE(alpha > 0.f, "%s: out_scale must be positive", what);
  if (w.route == WGRAD_ROWS) return wgrad16_rows<F16 != 0 ? 1 : 0>(what, w, big_split, small_split, dw_ref, g, ws, stream, F16 != 0 ? alpha : 1.f);
  constexpr unsigned main_tiles = T_SQUARE | T_N32;
  if constexpr (F16 != 0) {
    return plain5(g) ? wgrad16_t<ProbW16X, forms16<ProbW16X>(), main_tiles>(w, g, big_split, small_split, dw_ref, ws, stream, alpha, what)
                     : wgrad16_t<ProbW16KX, forms16<ProbW16KX>(), main_tiles>(w, g, big_split, small_split, dw_ref, ws, stream, alpha, what);
  } else {
    if (w.route == WGRAD_WIDE) {      // wide tiles / tap pairs
      constexpr unsigned pair_tiles = T64x64 | T128x128 | T64x128;
#define VP_W16(K5) (w.kind == 4 ? wgrad16_t<ProbW16T<K5, 0, false>, K32F, T64x128>(w, g, big_split, small_split, dw_ref, ws, stream, 1.f, what) \
                                : wgrad16_t<ProbW16T<K5, 0, true>, K32F, pair_tiles>(w, g, big_split, small_split, dw_ref, ws, stream, 1.f, what))
      return plain5(g) ? VP_W16(true) : VP_W16(false);
#undef VP_W16
    }
    return plain5(g) ? wgrad16_t<ProbW16, forms16<ProbW16>(), main_tiles>(w, g, big_split, small_split, dw_ref, ws, stream, 1.f, what)
                     : wgrad16_t<ProbW16K, forms16<ProbW16K>(), main_tiles>(w, g, big_split, small_split, dw_ref, ws, stream, 1.f, what);
  }
}
