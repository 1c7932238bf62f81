// Executes a gather / scatter ConvPlan (launch_plan.h) on igemm16_kernel, for every arithmetic and every epilogue: one descriptor
// filler and one dispatch per family, and the one "convolution + BatchNorm statistics" entry.  Templates only: a translation unit
// instantiates the kernels of the problem types P (and FORMS / TILES masks, igemm16.h) it names, nothing else.  DESIGN.md section 24.
#pragma once
#include <type_traits>
#include "common.h"
#include "igemm16p.h"

namespace vp {

constexpr unsigned FORMS_ALL = K64F | K32F | K64S | K32S, TILES_ALL = T_SQUARE | T_N32;

// What the epilogue does beyond storing the accumulators; a default-constructed one is "nothing".
struct ConvEpi {
  const float* bias = nullptr;      // per output channel (scatter family: the generic-geometry descriptors only)
  int act = VP_ACT_NONE;            // gather: none | sigmoid | relu; affine descriptors: none | relu
  float alpha = 1.f;                // multiplies the accumulators (fp16 planes: undoes a producer's scale)
  float* stat = nullptr;            // BatchNorm statistics slab (igemm16.h epilogue_stats32): K must not be split
  const float* scale = nullptr; const float* shift = nullptr; void* out_split = nullptr;      // is_affine<P> only (igemm16.h AffineEpi)
  int out_fmt = 0;                  // ... on fp16 planes: the format of out_split (AffineEpi::out_fmt)
};

// the pipelined kernel's descriptor (igemm16p.h) where ROUTE_PIPELINED exists for P: the plain 5x5 layers on bf16 pairs
template <class P> struct pipelined { using type = void; };
template <> struct pipelined<ProbF16> { using type = PF16; };
template <> struct pipelined<ProbT16> { using type = PT16; };

// The fp32 mode addresses its tensors in 16-bit units: the contracted channel count doubles and each operand is ONE plane.
template <class P> constexpr int units16() { return P::F32 ? 2 : 1; }
template <class P> constexpr size_t plane16(size_t elements) { return P::F32 ? 0 : elements; }

// what both families share: the weight planes, the output, the plan's split / tile order, the epilogue, the zero-fill and the dispatch
template <class P, unsigned FORMS, unsigned TILES>
static int conv_exec(const char* what, P& p, const ConvPlan& pl, const ConvGeom& g, const void* w, float* out, size_t n_out, const ConvEpi& e,
                     int ctile, hipStream_t s) {
  p.zero = vp_zero_page();
  p.w = (const u16*)w; p.w_plane = plane16<P>((size_t)g.Cs * g.Cb * g.nt);
  p.out = out; p.M = (int)pl.M; p.N = (int)pl.N;
  p.nsplit = pl.nsplit; p.xcd_map = pl.xcd_map;
  p.alpha = e.alpha; p.bias = e.bias; p.stat = e.stat;
  if constexpr (is_affine<P>::value) {
    p.e.scale = e.scale; p.e.shift = e.shift;
    p.e.out_split = (u16*)e.out_split; p.e.split_plane = n_out;
    p.e.relu = e.act == VP_ACT_RELU ? 1 : 0;
    p.e.out_fmt = e.out_fmt;
  }
  if (e.stat && pl.nsplit != 1) return fail(VP_ERR_ARG, "%s: this shape splits K", what);
  if (pl.zero_fill && hipMemsetAsync(out, 0, n_out * sizeof(float), s) != hipSuccess) return fail(VP_ERR_LAUNCH, "%s: memset failed", what);
  using Q = typename pipelined<P>::type;
  if constexpr (!std::is_void<Q>::value) {
    if (pl.route == ROUTE_PIPELINED) {
      Q q;
      static_cast<P&>(q) = p;
      launch_igemm16p(q, pl.kind, pl.M, pl.N, pl.gz, s, ctile, true, pl.m16);
      return check_launch(what);
    }
  }
  if (!launch_tiles16<P, FORMS, TILES>(p, pl.bm, pl.bn, pl.bk, pl.fast, pl.m16, pl.M, pl.N, pl.gz, s))
    return fail(VP_ERR_LAUNCH, "%s: no kernel for the planned %dx%d tile", what, pl.bm, pl.bn);
  return check_launch(what);
}

// `g` is the caller's geometry in elements; `big` / `w_p0`: split planes, or fp32 tensors for the fp32 mode
template <class P, unsigned FORMS, unsigned TILES>
static int conv_gather(const char* what, const ConvPlan& pl, const ConvGeom& g, const void* big, const void* w_p0, float* small_out,
                       const ConvEpi& e, vp_stream stream) {
  constexpr int U = units16<P>();
  P p;
  p.g = U == 1 ? g : make_geom(g.B, g.Hs, g.Ws, g.Cs, U * g.Cb, g.stride, g.ks, g.Hb, g.Wb);
  p.big = (const u16*)big; p.big_plane = plane16<P>((size_t)g.B * g.Hb * g.Wb * g.Cb);
  p.act = is_affine<P>::value ? VP_ACT_NONE : e.act;
  p.K = (int)pl.K; p.k_per_split = pl.k_per_split;
  return conv_exec<P, FORMS, TILES>(what, p, pl, g, w_p0, small_out, (size_t)pl.M * pl.N, e, g.Cb, (hipStream_t)stream);
}

template <class P, unsigned FORMS, unsigned TILES>
static int conv_scatter(const char* what, const ConvPlan& pl, const ConvGeom& g, const void* small, const void* w_p1, float* big_out,
                        const ConvEpi& e, vp_stream stream) {
  constexpr int U = units16<P>();
  P p;
  p.g = U == 1 ? g : make_geom(g.B, g.Hs, g.Ws, U * g.Cs, g.Cb, g.stride, g.ks, g.Hb, g.Wb);
  p.small = (const u16*)small; p.small_plane = plane16<P>((size_t)g.B * g.Hs * g.Ws * g.Cs);
  p.pair_phases = pl.pair_phases;
  return conv_exec<P, FORMS, TILES>(what, p, pl, g, w_p1, big_out, (size_t)g.B * g.Hb * g.Wb * g.Cb, e, g.Cs, (hipStream_t)stream);
}

// ---- BatchNorm statistics from the convolution epilogue -----------------------------------------------------------------
// A plain 5x5 layer on these kernels can emit {pivot, sum(x - pivot), sum((x - pivot)^2)} per (workgroup, output channel) from its
// accumulators (igemm16.h epilogue_stats32); one finaliser launch then produces mean / rstd / running statistics.  This replaces
// bn_partial_kernel<0>, i.e. one full read of the activation per BatchNorm layer.  The slab geometry is the launch's own ConvPlan
// (plan_stats, launch_plan.h); the finaliser reads it from there.
struct StatOut { float eps, momentum; float *mean, *rstd, *running_mean, *running_var; void* ws; size_t ws_bytes; };

// the finaliser for every arithmetic (conv16.hip, beside its kernel)
int stats_finish(const ConvPlan& pl, const StatOut& o, hipStream_t stream, const char* what);

// `run`: conv_gather / conv_scatter on the caller's descriptor type; `query`: the name of the arithmetic's workspace query;
// `aligned`: the fp32 plan depends on it, and only the staged route of the fp32 mode has the epilogue
using ConvRun = int (*)(const char*, const ConvPlan&, const ConvGeom&, const void*, const void*, float*, const ConvEpi&, vp_stream);
inline int conv5_stats(const char* what, const char* query, ConvRun run, int family, Arith ar, bool aligned, const void* a, const void* w,
                       float* out, int B, int Hs, int Ws, int Cbig, int Csmall, int stride, const StatOut& o, vp_stream stream) {
  VP_REQUIRE(a && w && out && o.mean && o.rstd && o.ws, "%s: null pointer", what);
  const ConvPlan pl = plan_stats(family, ar, B, Hs, Ws, Cbig, Csmall, stride, aligned, plan_switches());
  VP_REQUIRE(pl.stat_ok && (ar != F32 || pl.route == ROUTE_STAGED), "%s: this shape cannot emit statistics (%s() == 0)", what, query);
  if (o.ws_bytes < pl.stat_floats * sizeof(float)) return fail(VP_ERR_WORKSPACE, "%s: workspace too small", what);
  ConvEpi e;
  e.stat = (float*)o.ws;
  const int rc = run(what, pl, make_geom(B, Hs, Ws, Csmall, Cbig, stride, 5), a, w, out, e, stream);
  return rc ? rc : stats_finish(pl, o, (hipStream_t)stream, what);
}

}  // namespace vp
