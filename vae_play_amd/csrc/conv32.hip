// Exact-fp32 gather / scatter convolutions of the plain 5x5 layers on the split-operand kernel's data path (round 3).
//
// igemm.h (round 1) decomposes k -> (tap, channel) per 16-B load, predicates, walks K tap-major and never splits K: 41-70 % of the
// fp32-MFMA peak per layer (profiles/r03_*_f32).  igemm16_kernel already has what the 16-bit modes needed -- workgroup-uniform tap
// decomposition, the zero page, channel-chunk-major K order, XCD-aware tile order, 2-way split-K for the few-tile layers -- and its
// data path does not care what the 16-B chunks hold: MODE 3 (igemm16.h) stages ONE plane per operand, reads a fragment as 4 fp32 and
// contracts it with four v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate: the reference's arithmetic,
// models/networks.py:14,38).  The fp32 tensors are addressed in 16-bit units: [pixel][C] fp32 = [pixel][2C] u16, a 64-deep K-tile =
// 32 floats, so the gathered channel count is doubled in the geometry and nothing else changes.
#include "common.h"
#include "igemm16.h"
#include "conv32.h"

namespace vp {

int f32_fast_gather(const ConvPlan& pl, const float* big, const float* w_p0, const float* bias, float* out, const ConvGeom& g0, int act, hipStream_t s,
                    float* stat) {
  typedef ProbF16T<true, 3> P;
  P p;
  p.alpha = 1.f;
  p.zero = vp_zero_page();
  p.g = make_geom(g0.B, g0.Hs, g0.Ws, g0.Cs, 2 * g0.Cb, g0.stride, 5, g0.Hb, g0.Wb);      // gathered channels in 16-bit units
  p.big = (const u16*)big; p.big_plane = 0;
  p.w = (const u16*)w_p0; p.w_plane = 0;
  p.bias = bias; p.out = out; p.act = act;
  p.M = (int)pl.M; p.N = (int)pl.N; p.K = (int)pl.K;
  p.nsplit = pl.nsplit; p.k_per_split = pl.k_per_split; p.xcd_map = pl.xcd_map;
  p.stat = stat;
  if (stat && pl.nsplit != 1) return fail(VP_ERR_ARG, "vp_conv5_gather_stats_f32: this shape splits K");
  if (pl.zero_fill && hipMemsetAsync(out, 0, (size_t)pl.M * pl.N * sizeof(float), s) != hipSuccess) return fail(VP_ERR_LAUNCH, "vp_conv_gather_f32: memset failed");
  if (!launch_tiles16<P, K64F | K32F, T_SQUARE>(p, pl.bm, pl.bn, pl.bk, pl.fast, false, pl.M, pl.N, pl.gz, s))
    return fail(VP_ERR_LAUNCH, "vp_conv_gather_f32(fast): no kernel for the planned %dx%d tile", pl.bm, pl.bn);
  return check_launch("vp_conv_gather_f32(fast)");
}

int f32_fast_scatter(const ConvPlan& pl, const float* small, const float* w_p1, float* out, const ConvGeom& g0, hipStream_t s, float* stat) {
  typedef ProbT16T<true, 3> P;
  P p;
  p.alpha = 1.f;
  p.zero = vp_zero_page();
  p.g = make_geom(g0.B, g0.Hs, g0.Ws, 2 * g0.Cs, g0.Cb, g0.stride, 5, g0.Hb, g0.Wb);
  p.small = (const u16*)small; p.small_plane = 0;
  p.w = (const u16*)w_p1; p.w_plane = 0;
  p.out = out; p.M = (int)pl.M; p.N = (int)pl.N;
  p.nsplit = pl.nsplit; p.xcd_map = pl.xcd_map; p.pair_phases = pl.pair_phases;
  p.stat = stat;
  if (stat && pl.nsplit != 1) return fail(VP_ERR_ARG, "vp_conv5_scatter_stats_f32: this shape splits K");
  if (pl.zero_fill && hipMemsetAsync(out, 0, (size_t)g0.B * g0.Hb * g0.Wb * g0.Cb * sizeof(float), s) != hipSuccess)
    return fail(VP_ERR_LAUNCH, "vp_conv_scatter_f32: memset failed");
  if (!launch_tiles16<P, K64F | K32F, T_SQUARE>(p, pl.bm, pl.bn, pl.bk, pl.fast, false, pl.M, pl.N, pl.gz, s))
    return fail(VP_ERR_LAUNCH, "vp_conv_scatter_f32(fast): no kernel for the planned %dx%d tile", pl.bm, pl.bn);
  return check_launch("vp_conv_scatter_f32(fast)");
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

static bool aligned16(const void* a, const void* b) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }

int vp_conv5_gather_stats_f32(const float* big, const float* w_p0, float* small_out, int B, int Hs, int Ws, int Cbig, int Csmall, int stride,
                              float eps, float momentum, float* mean, float* rstd, float* running_mean, float* running_var, void* ws,
                              size_t ws_bytes, vp_stream stream) {
  VP_REQUIRE(big && w_p0 && small_out && mean && rstd && ws, "vp_conv5_gather_stats_f32: null pointer");
  const ConvPlan pl = plan_stats(0, F32, B, Hs, Ws, Cbig, Csmall, stride, aligned16(big, w_p0), plan_switches());
  VP_REQUIRE(pl.stat_ok && pl.route == ROUTE_STAGED, "vp_conv5_gather_stats_f32: this shape cannot emit statistics (vp_conv5_stats_f32_workspace_bytes() == 0)");
  if (ws_bytes < pl.stat_floats * sizeof(float)) return fail(VP_ERR_WORKSPACE, "vp_conv5_gather_stats_f32: workspace too small");
  int rc = f32_fast_gather(pl, big, w_p0, nullptr, small_out, make_geom(B, Hs, Ws, Csmall, Cbig, stride, 5), VP_ACT_NONE, (hipStream_t)stream, (float*)ws);
  if (rc) return rc;
  return stats_finish(pl, (const float*)ws, eps, momentum, mean, rstd, running_mean, running_var, (hipStream_t)stream, "vp_conv5_*_stats_f32(final)");
}

int vp_conv5_scatter_stats_f32(const float* small, const float* w_p1, float* big_out, int B, int Hs, int Ws, int Csmall, int Cbig, int stride,
                               float eps, float momentum, float* mean, float* rstd, float* running_mean, float* running_var, void* ws,
                               size_t ws_bytes, vp_stream stream) {
  VP_REQUIRE(small && w_p1 && big_out && mean && rstd && ws, "vp_conv5_scatter_stats_f32: null pointer");
  const ConvPlan pl = plan_stats(1, F32, B, Hs, Ws, Cbig, Csmall, stride, aligned16(small, w_p1), plan_switches());
  VP_REQUIRE(pl.stat_ok && pl.route == ROUTE_STAGED, "vp_conv5_scatter_stats_f32: this shape cannot emit statistics (vp_conv5_stats_f32_workspace_bytes() == 0)");
  if (ws_bytes < pl.stat_floats * sizeof(float)) return fail(VP_ERR_WORKSPACE, "vp_conv5_scatter_stats_f32: workspace too small");
  int rc = f32_fast_scatter(pl, small, w_p1, big_out, make_geom(B, Hs, Ws, Csmall, Cbig, stride, 5), (hipStream_t)stream, (float*)ws);
  if (rc) return rc;
  return stats_finish(pl, (const float*)ws, eps, momentum, mean, rstd, running_mean, running_var, (hipStream_t)stream, "vp_conv5_*_stats_f32(final)");
}

}
