// Shared by conv16.hip (bf16 pairs) and conv16_f16.hip (fp16 pairs): the templated launchers of the three split-operand families,
// which execute the plans of launch_plan.h.  Everything here is static / a template, so that each translation unit instantiates only the problem
// descriptors it dispatches (the fp16 modes live in their own object file: the two compile in parallel).
#pragma once
#include <type_traits>
#include "common.h"
#include "igemm16p.h"
#include "wgrad5.h"
#include "halo.h"
#include "narrow.h"
#include "split.h"
#include "conv32.h"

using namespace vp;


template <int F16> constexpr Arith arith16() { return F16 == 0 ? BF16X3 : (F16 == 2 ? F16_2 : F16_3); }

// The launchers execute a ConvPlan (launch_plan.h): descriptor from the geometry and the plan, the optional zero-fill, one dispatch.
template <class PF>
static int gather16_t(const ConvPlan& pl, const ConvGeom& g, const void* big_split, const void* w_p0_split, const float* bias, float* small_out,
                      int act, vp_stream stream, float* stat = nullptr, float alpha = 1.f) {
  PF p;
  p.alpha = alpha;
  p.zero = vp_zero_page();
  p.g = g;
  p.big = (const u16*)big_split; p.big_plane = (size_t)g.B * g.Hb * g.Wb * g.Cb;
  p.w = (const u16*)w_p0_split; p.w_plane = (size_t)g.Cs * g.Cb * g.nt;
  p.bias = bias; p.out = small_out; p.act = act;
  p.M = (int)pl.M; p.N = (int)pl.N; p.K = (int)pl.K;
  p.nsplit = pl.nsplit; p.k_per_split = pl.k_per_split; p.xcd_map = pl.xcd_map;
  p.stat = stat;
  if (stat && pl.nsplit != 1) return fail(VP_ERR_ARG, "vp_conv5_gather_stats_bf16x3: this shape splits K");
  if (pl.zero_fill && hipMemsetAsync(small_out, 0, (size_t)pl.M * pl.N * sizeof(float), (hipStream_t)stream) != hipSuccess)
    return fail(VP_ERR_LAUNCH, "vp_conv5_gather_bf16x3: memset failed");
  if constexpr (std::is_same<PF, ProbF16>::value) {
    if (pl.route == ROUTE_PIPELINED) {
      PF16 q;
      static_cast<ProbF16&>(q) = p;
      launch_igemm16p(q, pl.kind, pl.M, pl.N, pl.gz, (hipStream_t)stream, g.Cb, true, pl.m16);
      return check_launch("vp_conv_gather_bf16x3(pipelined)");
    }
  }
  if (!launch_tiles16<PF, K64F | K32F | K64S | K32S, T_SQUARE | T_N32>(p, pl.bm, pl.bn, pl.bk, pl.fast, pl.m16, pl.M, pl.N, pl.gz, (hipStream_t)stream))
    return fail(VP_ERR_LAUNCH, "vp_conv_gather_bf16x3: no kernel for the planned %dx%d tile", pl.bm, pl.bn);
  return check_launch("vp_conv_gather_bf16x3");
}

template <class PT>
static int scatter16_t(const ConvPlan& pl, const ConvGeom& g, const void* small_split, const void* w_p1_split, float* big_out, vp_stream stream,
                       float* stat = nullptr, float alpha = 1.f, const float* bias = nullptr) {
  PT p;
  p.alpha = alpha;
  p.bias = bias;
  p.zero = vp_zero_page();
  p.g = g;
  p.small = (const u16*)small_split; p.small_plane = (size_t)g.B * g.Hs * g.Ws * g.Cs;
  p.w = (const u16*)w_p1_split; p.w_plane = (size_t)g.Cs * g.Cb * g.nt;
  p.out = big_out; p.M = (int)pl.M; p.N = (int)pl.N;
  p.nsplit = pl.nsplit; p.xcd_map = pl.xcd_map;
  p.stat = stat;
  if (stat && pl.nsplit != 1) return fail(VP_ERR_ARG, "vp_conv5_scatter_stats_bf16x3: this shape splits K");
  if (pl.zero_fill && hipMemsetAsync(big_out, 0, (size_t)g.B * g.Hb * g.Wb * g.Cb * sizeof(float), (hipStream_t)stream) != hipSuccess)
    return fail(VP_ERR_LAUNCH, "vp_conv5_scatter_bf16x3: memset failed");
  if constexpr (std::is_same<PT, ProbT16>::value) {
    if (pl.route == ROUTE_PIPELINED) {
      PT16 q;
      static_cast<ProbT16&>(q) = p;
      launch_igemm16p(q, pl.kind, pl.M, pl.N, pl.gz, (hipStream_t)stream, g.Cs, true, pl.m16);
      return check_launch("vp_conv_scatter_bf16x3(pipelined)");
    }
  }
  p.pair_phases = pl.pair_phases;
  if (!launch_tiles16<PT, K64F | K32F | K64S | K32S, T_SQUARE | T_N32>(p, pl.bm, pl.bn, pl.bk, pl.fast, pl.m16, pl.M, pl.N, pl.gz, (hipStream_t)stream))
    return fail(VP_ERR_LAUNCH, "vp_conv_scatter_bf16x3: no kernel for the planned %dx%d tile", pl.bm, pl.bn);
  return check_launch("vp_conv_scatter_bf16x3");
}

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
static int wgrad16_rows(const WgradPlan& w, const void* big_split, const void* small_split, float* dw_ref, const ConvGeom& g, void* ws,
                        vp_stream stream, float alpha) {
  int slabs = 0;
  wgrad5_launch<MODE>(big_split, small_split, (float*)ws, g, w.kind, w.nsplit, w.k_per_split, alpha, (hipStream_t)stream, &slabs);
  int rc = check_launch("vp_conv_wgrad_bf16x3(rows of taps)");
  if (rc) return rc;
  return slab_reduce_launch((const float*)ws, dw_ref, g.Cs, g.Cb, slabs, (hipStream_t)stream, g.nt);
}

// ---- BatchNorm statistics from the convolution epilogue -----------------------------------------------------------------
// A 5x5 VAE layer on the split-operand kernels can emit {pivot, sum(x - pivot), sum((x - pivot)^2)} per (workgroup, output channel)
// from its accumulators (igemm16.h epilogue_stats32); one finaliser launch then produces mean / rstd / running statistics.
// This replaces bn_partial_kernel<0>, i.e. one full read of the activation per BatchNorm layer.  The slab geometry is the launch's own
// ConvPlan (plan_stats, launch_plan.h); the finaliser (stats_finish, conv32.h) reads it from there.

// ---- argument checks + dispatch of the three families; F16 = 0: bf16 pairs (three products), 2 | 3: fp16 pairs, products per fragment pair
template <int F16>
static int gather16(const void* big_split, const void* w_p0_split, const float* bias, float* small_out, int B, int Hs, int Ws, int Hb,
                    int Wb, int Cbig, int Csmall, int ks, int stride, int act, vp_stream stream, float alpha = 1.f) {
  VP_REQUIRE(big_split && w_p0_split && small_out, "vp_conv_gather_bf16x3: null pointer");
  VP_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Cbig > 0 && Csmall > 0 && Cbig % 8 == 0, "vp_conv_gather_bf16x3: Cbig must be a multiple of 8");
  VP_REQUIRE(stride == 1 || stride == 2, "vp_conv_gather_bf16x3: stride must be 1 or 2");
  VP_REQUIRE(ks == 1 || ks == 3 || ks == 4 || ks == 5, "vp_conv_gather_bf16x3: kernel size must be 1, 3, 4 or 5");
  VP_REQUIRE(act == VP_ACT_NONE || act == VP_ACT_SIGMOID, "vp_conv_gather_bf16x3: epilogue supports none|sigmoid");
  if constexpr (F16 != 0) VP_REQUIRE(alpha > 0.f, "vp_conv_gather_f16: out_scale must be positive");
  const ConvGeom g = make_geom(B, Hs, Ws, Csmall, Cbig, stride, ks, Hb, Wb);
  const ConvPlan pl = plan_conv(false, g, arith16<F16>(), bias != nullptr, act, true, EPI_NONE, plan_switches());
#define VP_G16(PF) gather16_t<PF>(pl, g, big_split, w_p0_split, bias, small_out, act, stream, nullptr, alpha)
  // fp16-pair planes, f16 = products per fragment pair: always the implicit-GEMM kernels (the halo kernels read bf16 pairs)
  if constexpr (F16 == 2) return plain5(g) ? VP_G16(ProbF16X) : VP_G16(ProbF16KX);
  else if constexpr (F16 == 3) return plain5(g) ? VP_G16(ProbF16H) : VP_G16(ProbF16KH);
  else {
    if (pl.route == ROUTE_HALO)
      return halo_gather_launch(pl.kind, big_split, w_p0_split, bias, small_out, B, Hs, Ws, Cbig, Csmall, stride, act, (hipStream_t)stream);
    return plain5(g) ? VP_G16(ProbF16) : VP_G16(ProbF16K);
  }
#undef VP_G16
}

template <int F16>
static int scatter16(const void* small_split, const void* w_p1_split, float* big_out, int B, int Hs, int Ws, int Hb, int Wb, int Csmall,
                     int Cbig, int ks, int stride, vp_stream stream, float alpha = 1.f, const float* bias = nullptr) {
  VP_REQUIRE(small_split && w_p1_split && big_out, "vp_conv_scatter_bf16x3: null pointer");
  VP_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Cbig > 0 && Csmall > 0 && Csmall % 8 == 0, "vp_conv_scatter_bf16x3: Csmall must be a multiple of 8");
  VP_REQUIRE(stride == 1 || stride == 2, "vp_conv_scatter_bf16x3: stride must be 1 or 2");
  VP_REQUIRE(ks == 1 || ks == 3 || ks == 4 || ks == 5, "vp_conv_scatter_bf16x3: kernel size must be 1, 3, 4 or 5");
  if constexpr (F16 != 0) VP_REQUIRE(alpha > 0.f, "vp_conv_scatter_f16: out_scale must be positive");
  const ConvGeom g = make_geom(B, Hs, Ws, Csmall, Cbig, stride, ks, Hb, Wb);
  const ConvPlan pl = plan_conv(true, g, arith16<F16>(), bias != nullptr, VP_ACT_NONE, true, EPI_NONE, plan_switches());
#define VP_S16(PT) scatter16_t<PT>(pl, g, small_split, w_p1_split, big_out, stream, nullptr, alpha, bias)
  if constexpr (F16 == 2) return plain5(g) ? VP_S16(ProbT16X) : VP_S16(ProbT16KX);
  else if constexpr (F16 == 3) return plain5(g) ? VP_S16(ProbT16H) : VP_S16(ProbT16KH);
  else {
    if (pl.route == ROUTE_HALO) return halo_scatter_launch(pl.kind, small_split, w_p1_split, big_out, B, Hs, Ws, Csmall, Cbig, (hipStream_t)stream);
    // with a bias (vp_conv_scatter_bias_bf16x3): always the generic-geometry kernel, whose epilogue adds it
    return (plain5(g) && !bias) ? VP_S16(ProbT16) : VP_S16(ProbT16K);
  }
#undef VP_S16
}

template <int F16>
static int wgrad16(const void* big_split, const void* small_split, float* dw_ref, int B, int Hs, int Ws, int Hb, int Wb, int Cbig,
                   int Csmall, int ks, int stride, void* ws, size_t ws_bytes, vp_stream stream, float alpha = 1.f, int max_cus = 0) {
  static_assert(F16 == 0 || F16 == 2, "weight gradients have no 3-product fp16 form");
  VP_REQUIRE(big_split && small_split && dw_ref && ws, "vp_conv_wgrad_bf16x3: null pointer");
  VP_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Cbig % 8 == 0 && Csmall % 8 == 0 && Cbig > 0 && Csmall > 0,
             "vp_conv_wgrad_bf16x3: channel counts must be multiples of 8");
  VP_REQUIRE(stride == 1 || stride == 2, "vp_conv_wgrad_bf16x3: stride must be 1 or 2");
  VP_REQUIRE(ks == 1 || ks == 3 || ks == 4 || ks == 5, "vp_conv_wgrad_bf16x3: kernel size must be 1, 3, 4 or 5");
  const ConvGeom g = make_geom(B, Hs, Ws, Csmall, Cbig, stride, ks, Hb, Wb);
  const WgradPlan w = plan_wgrad(g, arith16<F16>(), max_cus, ws_bytes, true, plan_switches());
  if (w.route == WGRAD_ROWS) {
    if constexpr (F16 != 0) VP_REQUIRE(alpha > 0.f, "vp_conv_wgrad_f16x2: out_scale must be positive");
  }
  if (ws_bytes / sizeof(float) < w.need_floats) return fail(VP_ERR_WORKSPACE, "vp_conv_wgrad_bf16x3: workspace too small");
  if constexpr (F16 != 0) VP_REQUIRE(alpha > 0.f, "vp_conv_wgrad_f16x2: out_scale must be positive");
  if (w.route == WGRAD_ROWS) return wgrad16_rows<F16 != 0 ? 1 : 0>(w, big_split, small_split, dw_ref, g, ws, stream, F16 != 0 ? alpha : 1.f);
  constexpr unsigned main_tiles = T_SQUARE | T_N32;
  if constexpr (F16 != 0) {
    const char* what = "vp_conv_wgrad_bf16x3(main)";
    return plain5(g) ? wgrad16_t<ProbW16X, forms16<ProbW16X>(), main_tiles>(w, g, big_split, small_split, dw_ref, ws, stream, alpha, what)
                     : wgrad16_t<ProbW16KX, forms16<ProbW16KX>(), main_tiles>(w, g, big_split, small_split, dw_ref, ws, stream, alpha, what);
  } else {
    if (w.route == WGRAD_WIDE) {
      const char* what = "vp_conv_wgrad_bf16x3(wide tiles / tap pairs)";
      constexpr unsigned pair_tiles = T64x64 | T128x128 | T64x128;
#define VP_W16(K5) (w.kind == 4 ? wgrad16_t<ProbW16T<K5, 0, false>, K32F, T64x128>(w, g, big_split, small_split, dw_ref, ws, stream, 1.f, what) \
                                : wgrad16_t<ProbW16T<K5, 0, true>, K32F, pair_tiles>(w, g, big_split, small_split, dw_ref, ws, stream, 1.f, what))
      return plain5(g) ? VP_W16(true) : VP_W16(false);
#undef VP_W16
    }
    const char* what = "vp_conv_wgrad_bf16x3(main)";
    return plain5(g) ? wgrad16_t<ProbW16, forms16<ProbW16>(), main_tiles>(w, g, big_split, small_split, dw_ref, ws, stream, 1.f, what)
                     : wgrad16_t<ProbW16K, forms16<ProbW16K>(), main_tiles>(w, g, big_split, small_split, dw_ref, ws, stream, 1.f, what);
  }
}
