// BatchNorm (+ activation) over an [R][C] NHWC view.  HBM-bound: every pass streams the
// activation once with 16-B loads; reductions are per-thread fp32 partials -> LDS tree ->
// per-chunk slab -> fp64 finalize (deterministic, no atomics).
//   R = B*H*W for BatchNorm2d, R = B for BatchNorm1d (models/networks.py:16,40,66,89).
// The building blocks every kernel below shares are stated once, up front: the row walk (walk_rows), the
// per-thread channel constants (chan_const), the block column sum (block_colsum), the statistics finalisation (bn_finalize) and the
// backward expressions (bn_g, bn_dx); the host side has one workspace layout (bn_ws) and one launcher per stage.
#include <stdlib.h>
#include "common.h"
#include "problems.h"
#include "split.h"

namespace vp {

constexpr int BN_TX = 16;   // float4 lanes across channels  (64 channels per block)
constexpr int BN_TY = 16;   // row lanes
constexpr int BN_CH = BN_TX * 4;

struct BnGrid { int chunks_r, chunks_c, rows_per_chunk; };

inline BnGrid bn_grid(int R, int C) {
  BnGrid g;
  g.chunks_c = (C + BN_CH - 1) / BN_CH;
  int total = 1024;
  int want = total / g.chunks_c;
  if (want < 1) want = 1;
  int maxr = (R + 63) / 64;   // at least ~64 rows per chunk
  if (maxr < 1) maxr = 1;
  g.chunks_r = want < maxr ? want : maxr;
  g.rows_per_chunk = (R + g.chunks_r - 1) / g.chunks_r;
  g.chunks_r = (R + g.rows_per_chunk - 1) / g.rows_per_chunk;
  return g;
}

__device__ __forceinline__ float act_apply(float v, int act, float slope) {
  switch (act) {
    case ACT_RELU: return v > 0.f ? v : 0.f;
    case ACT_LRELU: return v > 0.f ? v : v * slope;
    case ACT_TANH: return tanhf(v);
    case ACT_SIGMOID: return 1.f / (1.f + __expf(-v));
    default: return v;
  }
}
// pre-activation of the normalised value: gamma * ((x - mean) * rstd) + beta, written ONCE so that forward and backward
// round it identically (the backward kernels rebuild the activation mask from it).  The hoisted form x * scale + shift
// with shift = beta - mean * scale cancels two terms of size |mean| / sigma: for Linear -> BatchNorm1d over a few similar
// samples (|mean| / sigma ~ 1e3) that cost three digits of y and made the VAE-GAN gradients 10-50 x noisier than torch's.
__device__ __forceinline__ float bn_pre(float x, float mu, float rs, float ga, float be) {
  return fmaf(ga, (x - mu) * rs, be);
}
// derivative of act at pre-activation value u
__device__ __forceinline__ float act_grad_pre(float u, int act, float slope) {
  switch (act) {
    case ACT_RELU: return u > 0.f ? 1.f : 0.f;
    case ACT_LRELU: return u > 0.f ? 1.f : slope;
    case ACT_TANH: { float t = tanhf(u); return 1.f - t * t; }
    case ACT_SIGMOID: { float s = 1.f / (1.f + __expf(-u)); return s * (1.f - s); }
    default: return 1.f;
  }
}
// derivative of act at the activation's own output v
__device__ __forceinline__ float act_grad_from_y(float v, int act, float slope) {
  switch (act) {
    case ACT_RELU: return v > 0.f ? 1.f : 0.f;
    case ACT_LRELU: return v > 0.f ? 1.f : slope;
    case ACT_TANH: return 1.f - v * v;
    case ACT_SIGMOID: return v * (1.f - v);
    default: return 1.f;
  }
}

// ---- the shared pieces ---------------------------------------------------------------------------------------------------------------
// 4 consecutive floats: one 16-B access when vec, else element by element over the nv (< 4 at the last quad) that exist
__device__ __forceinline__ vp_f32x4 ld4(const float* __restrict__ p, bool vec, int nv) {
  if (vec) return *reinterpret_cast<const vp_f32x4*>(p);
  vp_f32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : 0.f;
  return v;
}
__device__ __forceinline__ void ld4(float (&v)[4], const float* __restrict__ p, bool vec, int nv) {
  const vp_f32x4 t = ld4(p, vec, nv);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = t[j];
}
__device__ __forceinline__ void st4(float* __restrict__ p, const vp_f32x4& v, bool vec, int nv) {
  if (vec) { *reinterpret_cast<vp_f32x4*>(p) = v; return; }
#pragma unroll
  for (int j = 0; j < 4; ++j) if (j < nv) p[j] = v[j];
}

// What one thread holds of one row: N quads (x | x, dy | branch 1, branch 2 | branch 1, branch 2, dy), as floats: kept as the
// 16-B vectors they were loaded as, the tiled backward kernel takes 16 more VGPRs and two others lose a wave of occupancy.
template <int N> struct Row { float v[N][4]; };

// THE row walk: a thread visits rows r, r + 16, ... < r1.  U rows per trip with all of the trip's loads issued before the first use
// (one load per trip left the small layers at 2-3 TB/s), consumed in row order, then a one-row tail: sums taken in use() see the rows
// in the same order whatever U is.  trips = false (element-wise loads) walks row by row.
template <int U, class Load, class Use>
__device__ __forceinline__ void walk_rows(int r, int r1, bool trips, Load load, Use use) {
  if (trips) {
    for (; r + (U - 1) * BN_TY < r1; r += U * BN_TY) {
      decltype(load(r)) v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = load(r + u * BN_TY);
#pragma unroll
      for (int u = 0; u < U; ++u) use(r + u * BN_TY, v[u]);
    }
  }
  for (; r < r1; r += BN_TY) use(r, load(r));
}

// Per-thread constants of a thread's 4 channels c .. c + 3, of which the first nv exist (nv <= 0: none, and then mean and rstd are
// not touched).  A channel outside nv gives mean 0, rstd 0, gamma 1, beta 0; so does a null gamma or beta.
struct ChanConst { float mu[4], rs[4], ga[4], be[4]; };
__device__ __forceinline__ ChanConst chan_const(const float* __restrict__ mean, const float* __restrict__ rstd,
                                                const float* __restrict__ gamma, const float* __restrict__ beta, int c, int nv) {
  ChanConst k;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool ok = j < nv;
    k.mu[j] = ok ? mean[c + j] : 0.f;
    k.rs[j] = ok ? rstd[c + j] : 0.f;
    k.ga[j] = (ok && gamma) ? gamma[c + j] : 1.f;
    k.be[j] = (ok && beta) ? beta[c + j] : 0.f;
  }
  return k;
}

// One more term of a pair of running sums (sum a, sum a * b): (x - pivot, its square) or (g, g * xhat).  The fma is explicit; the compiler
// may still contract `sa += a` with the multiplication that made a (DESIGN.md section 23 on what that means for the pair blend).
__device__ __forceinline__ void sum_pair(float& sa, float& sab, float a, float b) {
  sa += a;
  sab = fmaf(a, b, sab);
}

// Block column sum of N running sums: every thread (tx, ty) of the 16 x 16 map hands in s[q][0..3] for its 4 channels; thread t <
// N * 64 gets back sum q = t / 64 of the block's channel cc = t % 64, added over the 16 row lanes in lane order (other threads: 0).
template <int N>
__device__ __forceinline__ float block_colsum(const float (&s)[N][4]) {
  __shared__ float sh[N][BN_TY][BN_CH + 4];
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) sh[q][ty][tx * 4 + j] = s[q][j];
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x < N * BN_CH) {
    const int q = threadIdx.x / BN_CH, cc = threadIdx.x % BN_CH;
#pragma unroll
    for (int k = 0; k < BN_TY; ++k) t += sh[q][k][cc];
  }
  return t;
}

// Statistics of one channel from the fp64 sums s = sum (x - pivot), q = sum (x - pivot)^2 over R rows: mean, rstd, and the running
// statistics (momentum-weighted, the variance unbiased) where given.
__device__ __forceinline__ void bn_finalize(double s, double q, int R, float pivot, float eps, float momentum, float& mean, float& rstd,
                                            float* __restrict__ rm, float* __restrict__ rv) {
  const double ms = s / R;                 // mean of (x - pivot)
  double var = q / R - ms * ms;
  if (var < 0.0) var = 0.0;
  const double m = (double)pivot + ms;
  mean = (float)m;
  rstd = (float)(1.0 / sqrt(var + (double)eps));
  if (rm) *rm = (1.f - momentum) * *rm + momentum * (float)m;
  if (rv) {
    const double unb = R > 1 ? var * (double)R / (double)(R - 1) : var;
    *rv = (1.f - momentum) * *rv + momentum * (float)unb;
  }
}

// g = dy * act'(gamma * xhat + beta)
__device__ __forceinline__ float bn_g(float dy, float xh, float ga, float be, int act, float slope) {
  return dy * act_grad_pre(fmaf(ga, xh, be), act, slope);
}
// dx = gamma * rstd * (g - (k0 + xhat * k1)) with k0 = sum_g / R, k1 = sum_gx / R (both 0 without batch statistics)
__device__ __forceinline__ float bn_dx(float ga, float rs, float g, float xh, float k0, float k1) {
  return ga * rs * (g - fmaf(xh, k1, k0));
}

// MODE 0: (sum x, sum x^2).  MODE 1: (sum g, sum g*xhat) with g = dy * act'(gamma*xhat+beta).
template <int MODE>
__global__ void __launch_bounds__(256) bn_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ part, int R, int C, int rows_per_chunk,
                                                         int act, float slope, size_t bxs, size_t bps) {
  // blockIdx.z = image index of a batched (InstanceNorm) call: bxs elements per image, bps partial floats per image
  x += blockIdx.z * bxs; part += blockIdx.z * bps;
  if (MODE == 1) { dy += blockIdx.z * bxs; mean += blockIdx.z * (size_t)C; rstd += blockIdx.z * (size_t)C; }
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
  const int c = blockIdx.y * BN_CH + tx * 4;
  const int r0 = blockIdx.x * rows_per_chunk;
  const int r1 = min(R, r0 + rows_per_chunk);
  float s[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const bool vec = (C % 4 == 0);
  const int nv = C - c;
  // MODE 0 sums (x - pivot) and (x - pivot)^2 with pivot = the channel's value in row 0, held in mu (bn_finalize adds it back):
  // E[x^2] - E[x]^2 on raw values loses log2(mean^2 / var) bits, which for a Linear -> BatchNorm1d over a batch of 4
  // similar images (mean^2 / var ~ 1e3-1e4) turned 2e-7 of input rounding into 1e-3 of sigma
  const ChanConst k = MODE == 0 ? chan_const(x, x, nullptr, nullptr, c, nv) : chan_const(mean, rstd, gamma, beta, c, nv);
  if (c < C) {
    constexpr int N = MODE == 0 ? 1 : 2;
    // 4 (MODE 0) or 8 (MODE 1) independent 16-B loads in flight
    walk_rows<4>(r0 + ty, r1, vec,
      [&](int r) {
        const size_t off = (size_t)r * C + c;
        Row<N> v;
        ld4(v.v[0], x + off, vec, nv);
        if (MODE == 1) ld4(v.v[N - 1], dy + off, vec, nv);
        return v;
      },
      [&](int, const Row<N>& v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (MODE == 0) {
            const float d = v.v[0][j] - k.mu[j];
            sum_pair(s[0][j], s[1][j], d, d);
          } else {
            const float xh = (v.v[0][j] - k.mu[j]) * k.rs[j];
            sum_pair(s[0][j], s[1][j], bn_g(v.v[N - 1][j], xh, k.ga[j], k.be[j], act, slope), xh);
          }
        }
      });
  }
  const float t = block_colsum<2>(s);
  if (threadIdx.x < 2 * BN_CH) {
    const int which = threadIdx.x / BN_CH, cg = blockIdx.y * BN_CH + threadIdx.x % BN_CH;
    if (cg < C) part[((size_t)which * gridDim.x + blockIdx.x) * C + cg] = t;
  }
}

// Finalize: 4 channels per 256-thread block, one wavefront (64 lanes) per channel; each lane sums every
// 64th chunk partial in fp64 with two independent chains, then a shuffle reduction.  (The first version,
// one thread per channel looping over up to 2048 chunks, cost 185 us per call; 16 lanes per channel
// still 9.5 us.)
constexpr int FIN_C = 4;

__device__ __forceinline__ void bn_final_reduce(const float* __restrict__ part, int nchunk, int C, int c, int lane,
                                                double& s, double& q) {
  double s0 = 0.0, s1 = 0.0, q0 = 0.0, q1 = 0.0;
  if (c < C) {
    int k = lane;
    for (; k + 64 < nchunk; k += 128) {
      s0 += (double)part[(size_t)k * C + c];
      s1 += (double)part[(size_t)(k + 64) * C + c];
      q0 += (double)part[((size_t)nchunk + k) * C + c];
      q1 += (double)part[((size_t)nchunk + k + 64) * C + c];
    }
    if (k < nchunk) {
      s0 += (double)part[(size_t)k * C + c];
      q0 += (double)part[((size_t)nchunk + k) * C + c];
    }
  }
  s = wave_sum_d(s0 + s1);
  q = wave_sum_d(q0 + q1);
}

__global__ void __launch_bounds__(256) bn_stats_final_kernel(const float* __restrict__ part, int nchunk, int R, int C, float eps,
                                                             float momentum, float* __restrict__ mean, float* __restrict__ rstd,
                                                             float* __restrict__ rm, float* __restrict__ rv, const float* __restrict__ x,
                                                             size_t bps, size_t bxs) {
  part += blockIdx.z * bps; mean += blockIdx.z * (size_t)C; rstd += blockIdx.z * (size_t)C; x += blockIdx.z * bxs;
  const int c = blockIdx.x * FIN_C + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  double s, q;
  bn_final_reduce(part, nchunk, C, c, lane, s, q);
  if (lane != 0 || c >= C) return;
  bn_finalize(s, q, R, x[c], eps, momentum, mean[c], rstd[c], rm ? rm + c : nullptr, rv ? rv + c : nullptr);   // pivot = x[row 0][c]
}

__global__ void __launch_bounds__(256) bn_bwd_final_kernel(const float* __restrict__ part, int nchunk, int C,
                                                           float* __restrict__ sum_g, float* __restrict__ sum_gx,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, size_t bps) {
  part += blockIdx.z * bps; sum_g += blockIdx.z * (size_t)C; sum_gx += blockIdx.z * (size_t)C;
  const int c = blockIdx.x * FIN_C + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  double s, q;
  bn_final_reduce(part, nchunk, C, c, lane, s, q);
  if (lane != 0 || c >= C) return;
  sum_g[c] = (float)s;
  sum_gx[c] = (float)q;
  if (dbeta) dbeta[c] = (float)s;
  if (dgamma) dgamma[c] = (float)q;
}

// ---- flat passes for C % 4 != 0, one element per thread and trip: no split planes (they need C % 4 == 0), so no saturation flag
// y = act(gamma * (x - mean) * rstd + beta)
__global__ void __launch_bounds__(256) bn_act_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ y, size_t n,
                                                         int C, int act, float slope, size_t bxs) {
  x += blockIdx.z * bxs; y += blockIdx.z * bxs; mean += blockIdx.z * (size_t)C; rstd += blockIdx.z * (size_t)C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    y[i] = act_apply(bn_pre(x[i], mean[c], rstd[c], gamma ? gamma[c] : 1.f, beta ? beta[c] : 0.f), act, slope);
  }
}

// dx = gamma*rstd*(g - [batch_stats]*(sum_g + xhat*sum_gx)/R): summed and scaled in this order, not bn_dx's fma of pre-scaled sums,
// so this path and the tiled one may differ in the last bit
__global__ void __launch_bounds__(256) bn_act_bwd_kernel(const float* __restrict__ x, const float* dy,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ sum_g, const float* __restrict__ sum_gx,
                                                         float* dx, size_t n, int C, float invR, int act,
                                                         float slope, size_t bxs) {
  x += blockIdx.z * bxs; dy += blockIdx.z * bxs; dx += blockIdx.z * bxs; mean += blockIdx.z * (size_t)C; rstd += blockIdx.z * (size_t)C;
  sum_g += blockIdx.z * (size_t)C; sum_gx += blockIdx.z * (size_t)C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const float ga = gamma ? gamma[c] : 1.f, be = beta ? beta[c] : 0.f;
    const float xh = (x[i] - mean[c]) * rstd[c];
    const float g = bn_g(dy[i], xh, ga, be, act, slope);
    dx[i] = ga * rstd[c] * (g - (sum_g[c] + xh * sum_gx[c]) * invR);
  }
}

__global__ void act_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n, int act, float slope) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    y[i] = act_apply(x[i], act, slope);
}
__global__ void act_bwd_from_y_kernel(const float* __restrict__ y, const float* dy, float* dx,
                                      size_t n, int act, float slope) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dx[i] = dy[i] * act_grad_from_y(y[i], act, slope);
}

// ---- fast paths for C % 4 == 0: same (16 float4 columns x 16 rows) thread map as bn_partial_kernel, so the
// per-channel constants are computed once per thread instead of once per element, and every 16-lane
// group streams 256 contiguous bytes per row.
__global__ void __launch_bounds__(256) bn_act_fwd_tiled_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* __restrict__ y,
                                                               u16_t* __restrict__ y_split, int ldy, int R, int C,
                                                               int rows_per_chunk, int act, float slope, size_t bxs, int sfmt) {
  // ldy = floats between two rows of y (C: dense; more: y is a channel slice of a wider NHWC buffer); the planes stay dense
  x += blockIdx.z * bxs; mean += blockIdx.z * (size_t)C; rstd += blockIdx.z * (size_t)C;
  if (y) y += blockIdx.z * (size_t)R * ldy;
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
  const int c = blockIdx.y * BN_CH + tx * 4;
  if (c >= C) return;
  const ChanConst k = chan_const(mean, rstd, gamma, beta, c, 4);
  const int r0 = blockIdx.x * rows_per_chunk;
  const int r1 = min(R, r0 + rows_per_chunk);
  // split planes span all images of a batched (InstanceNorm) launch: plane = gridDim.z * R * C elements, image z at z * bxs
  const size_t n = (size_t)R * C * gridDim.z;
  if (y_split) y_split += blockIdx.z * bxs;
  walk_rows<4>(r0 + ty, r1, true,                       // four independent 16-B loads in flight
    [&](int r) { Row<1> v; ld4(v.v[0], x + (size_t)r * C + c, true, 4); return v; },
    [&](int r, const Row<1>& v) {
      const size_t off = (size_t)r * C + c;
      vp_f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = act_apply(bn_pre(v.v[0][j], k.mu[j], k.rs[j], k.ga[j], k.be[j]), act, slope);
      if (y) *reinterpret_cast<vp_f32x4*>(y + (size_t)r * ldy + c) = o;
      if (y_split) store_split4(y_split, n, off, o[0], o[1], o[2], o[3], sfmt);
    });
}

__global__ void __launch_bounds__(256) bn_act_bwd_tiled_kernel(const float* __restrict__ x, const float* dy,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ sum_g, const float* __restrict__ sum_gx,
                                                               float* dx, u16_t* __restrict__ dx_split, int R, int C,
                                                               int rows_per_chunk, float invR, int act, float slope,
                                                               size_t bxs, int sfmt, float sscale, int* __restrict__ sat) {
  x += blockIdx.z * bxs; dy += blockIdx.z * bxs; mean += blockIdx.z * (size_t)C; rstd += blockIdx.z * (size_t)C;
  sum_g += blockIdx.z * (size_t)C; sum_gx += blockIdx.z * (size_t)C;
  if (dx) dx += blockIdx.z * bxs;
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
  const int c = blockIdx.y * BN_CH + tx * 4;
  if (c >= C) return;
  const ChanConst k = chan_const(mean, rstd, gamma, beta, c, 4);
  float k0[4], k1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { k0[j] = sum_g[c + j] * invR; k1[j] = sum_gx[c + j] * invR; }
  const int r0 = blockIdx.x * rows_per_chunk;
  const int r1 = min(R, r0 + rows_per_chunk);
  const size_t n = (size_t)R * C * gridDim.z;          // (batched launch: see bn_act_fwd_tiled_kernel)
  if (dx_split) dx_split += blockIdx.z * bxs;
  walk_rows<4>(r0 + ty, r1, true,                       // eight independent 16-B loads in flight
    [&](int r) {
      const size_t off = (size_t)r * C + c;
      Row<2> v;
      ld4(v.v[0], x + off, true, 4);
      ld4(v.v[1], dy + off, true, 4);
      return v;
    },
    [&](int r, const Row<2>& v) {
      const size_t off = (size_t)r * C + c;
      vp_f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xh = (v.v[0][j] - k.mu[j]) * k.rs[j];
        o[j] = bn_dx(k.ga[j], k.rs[j], bn_g(v.v[1][j], xh, k.ga[j], k.be[j], act, slope), xh, k0[j], k1[j]);
      }
      if (dx) *reinterpret_cast<vp_f32x4*>(dx + off) = o;
      if (dx_split) store_split4(dx_split, n, off, o[0] * sscale, o[1] * sscale, o[2] * sscale, o[3] * sscale, sfmt);
      // fp16 pairs clamp at +-65504 (split.h): tell the caller that a scaled gradient left fp16's range (a sticky flag, any writer wins)
      if (sat && sfmt == SPLIT_F16 &&
          fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fmaxf(fabsf(o[2]), fabsf(o[3]))) * sscale > 65504.f) *sat = 1;
    });
}

// elementwise passes want more, smaller chunks than the reductions (no partial slabs to combine)
inline BnGrid bn_apply_grid(int R, int C) {
  BnGrid g;
  g.chunks_c = (C + BN_CH - 1) / BN_CH;
  int total = 4096;
  int rows_min = 4;                                                     // trips of 16 rows per workgroup, at least
  int want = total / g.chunks_c;
  if (want < 1) want = 1;
  int maxr = (R + BN_TY * rows_min - 1) / (BN_TY * rows_min);
  g.chunks_r = want < maxr ? want : maxr;
  if (g.chunks_r < 1) g.chunks_r = 1;
  g.rows_per_chunk = (R + g.chunks_r - 1) / g.chunks_r;
  g.chunks_r = (R + g.rows_per_chunk - 1) / g.rows_per_chunk;
  return g;
}


// ---- BatchNorm over a handful of rows (the dense layers: R = batch <= 64) in ONE launch --------------------------------------------
// nn.BatchNorm1d + F.relu behind nn.Linear (models/networks.py:66-67,89-90) normalises over the batch only: the three-launch form
// (partial sums, finaliser, apply) is pure launch latency there (3 x ~6 us for 32 rows).  One workgroup owns 64 channels and all
// rows; a thread keeps its <= 4 rows of 4 channels in registers.  The arithmetic is the three-launch path's, step for step, through
// the same functions (sum_pair in the same order, block_colsum, bn_finalize, bn_pre, bn_g, bn_dx), so results are bit-identical to it.
constexpr int BN_SMALL_R = 4 * BN_TY;       // 64 rows

__global__ void __launch_bounds__(256) bn_small_fwd_kernel(const float* __restrict__ x, int R, int C, float eps, float momentum,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ rm,
                                                           float* __restrict__ rv, float* __restrict__ y, int act, float slope) {
  __shared__ float fin[2][BN_CH];
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
  const int c = blockIdx.x * BN_CH + tx * 4;
  const bool cok = c < C;                     // C % 4 == 0: a quad is inside or outside
  float xv[4][4];
  const ChanConst pv = chan_const(x, x, nullptr, nullptr, c, cok ? 4 : 0);                 // mu = pivot = row 0
  float s[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = ty + BN_TY * i;
    if (cok && r < R) {
      ld4(xv[i], x + (size_t)r * C + c, true, 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = xv[i][j] - pv.mu[j]; sum_pair(s[0][j], s[1][j], d, d); }
    }
  }
  const float t = block_colsum<2>(s);
  if (threadIdx.x < 2 * BN_CH) fin[threadIdx.x / BN_CH][threadIdx.x % BN_CH] = t;
  __syncthreads();
  if (threadIdx.x < BN_CH) {
    const int cc = threadIdx.x, cg = blockIdx.x * BN_CH + cc;
    if (cg < C) {
      float mf, rf;
      bn_finalize((double)fin[0][cc], (double)fin[1][cc], R, x[cg], eps, momentum, mf, rf, rm ? rm + cg : nullptr, rv ? rv + cg : nullptr);
      mean[cg] = mf;
      rstd[cg] = rf;
      fin[0][cc] = mf;
      fin[1][cc] = rf;
    }
  }
  __syncthreads();
  if (!cok || !y) return;
  ChanConst k = chan_const(mean, rstd, gamma, beta, c, 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { k.mu[j] = fin[0][tx * 4 + j]; k.rs[j] = fin[1][tx * 4 + j]; }     // as this block finalised them, from LDS
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = ty + BN_TY * i;
    if (r < R) {
      vp_f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = act_apply(bn_pre(xv[i][j], k.mu[j], k.rs[j], k.ga[j], k.be[j]), act, slope);
      *reinterpret_cast<vp_f32x4*>(y + (size_t)r * C + c) = o;
    }
  }
}

__global__ void __launch_bounds__(256) bn_small_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           int R, int C, float invR, int act, float slope) {
  __shared__ float fin[2][BN_CH];
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
  const int c = blockIdx.x * BN_CH + tx * 4;
  const bool cok = c < C;
  const ChanConst k = chan_const(mean, rstd, gamma, beta, c, cok ? 4 : 0);
  float gq[4][4], xh[4][4];
  float s[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = ty + BN_TY * i;
    if (cok && r < R) {
      float xv[4], dv[4];
      ld4(xv, x + (size_t)r * C + c, true, 4);
      ld4(dv, dy + (size_t)r * C + c, true, 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xh[i][j] = (xv[j] - k.mu[j]) * k.rs[j];
        gq[i][j] = bn_g(dv[j], xh[i][j], k.ga[j], k.be[j], act, slope);
        sum_pair(s[0][j], s[1][j], gq[i][j], xh[i][j]);
      }
    }
  }
  const float t = block_colsum<2>(s);
  if (threadIdx.x < 2 * BN_CH) {
    const int which = threadIdx.x / BN_CH, cc = threadIdx.x % BN_CH;
    fin[which][cc] = t;
    const int cg = blockIdx.x * BN_CH + cc;
    if (cg < C) {
      if (which == 0 && dbeta) dbeta[cg] = t;
      if (which == 1 && dgamma) dgamma[cg] = t;
    }
  }
  __syncthreads();
  if (!cok) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = ty + BN_TY * i;
    if (r < R) {
      vp_f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = bn_dx(k.ga[j], k.rs[j], gq[i][j], xh[i][j], fin[0][tx * 4 + j] * invR, fin[1][tx * 4 + j] * invR);
      *reinterpret_cast<vp_f32x4*>(dx + (size_t)r * C + c) = o;
    }
  }
}

// ---- label-gated pair of convolutions (models/network_Style_GAN.py:72-79) -----------------------------------------------------------
// u [B][R][2C] is the output of ONE convolution whose weights are conv_1's and conv_2's stacked along the output channel: channels
// [0, C) are branch 1, [C, 2C) branch 2.  y[b][r][c] = w1 * act(pre(u[b][r][c])) + w2 * act(pre(u[b][r][C + c])) with w2 = label[b],
// w1 = 1 - label[b] and pre = InstanceNorm (norm = 1: the statistics are the InstanceNorm kernels above run over 2C channels) or the
// identity (norm = 0).  Same (16 float4 columns x 16 rows) thread map as the tiled kernels above, over the C output channels; VEC =
// (C % 4 == 0) takes 16-B loads and stores, the other instantiation guards every element.  A branch's per-thread constants are a
// ChanConst of its mean and rstd (gamma 1, beta 0; nothing is loaded when norm = 0, where they are not used).
// pre-activation value, as the forward computes it (the backward rebuilds the activation mask from the same expression)
__device__ __forceinline__ float pair_pre(float v, float mu, float rs, int norm) { return norm ? bn_pre(v, mu, rs, 1.f, 0.f) : v; }
// g = w * dy * act'(pre): one expression for the partial sums and the apply pass
__device__ __forceinline__ float pair_g(float w, float d, float pre, int act, float slope) { return (w * d) * act_grad_pre(pre, act, slope); }

template <bool VEC>
__global__ void __launch_bounds__(256) pair_blend_fwd_kernel(const float* __restrict__ u, const float* __restrict__ label,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             float* __restrict__ y, u16_t* __restrict__ y_split, int R, int C,
                                                             int rows_per_chunk, int norm, int act, float slope) {
  const int b = blockIdx.z, C2 = 2 * C;
  const size_t bys = (size_t)R * C;
  u += (size_t)b * 2 * bys; y += (size_t)b * bys;
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
  const int c = blockIdx.y * BN_CH + tx * 4;
  if (c >= C) return;
  const int nv = min(4, C - c);
  const float w2 = label[b], w1 = 1.f - w2;
  mean += (size_t)b * C2; rstd += (size_t)b * C2;
  const ChanConst s1 = chan_const(mean, rstd, nullptr, nullptr, c, norm ? nv : 0);
  const ChanConst s2 = chan_const(mean, rstd, nullptr, nullptr, C + c, norm ? nv : 0);
  const size_t n = bys * gridDim.z;                   // one split plane spans all images
  if (y_split) y_split += (size_t)b * bys;
  const int r0 = blockIdx.x * rows_per_chunk;
  const int r1 = min(R, r0 + rows_per_chunk);
  walk_rows<4>(r0 + ty, r1, true,                     // eight independent loads in flight
    [&](int r) {
      const float* p = u + (size_t)r * C2 + c;
      Row<2> v;
      ld4(v.v[0], p, VEC, nv);
      ld4(v.v[1], p + C, VEC, nv);
      return v;
    },
    [&](int r, const Row<2>& v) {
      vp_f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float a1 = act_apply(pair_pre(v.v[0][j], s1.mu[j], s1.rs[j], norm), act, slope);
        const float a2 = act_apply(pair_pre(v.v[1][j], s2.mu[j], s2.rs[j], norm), act, slope);
        o[j] = fmaf(w2, a2, w1 * a1);
      }
      const size_t off = (size_t)r * C + c;
      st4(y + off, o, VEC, nv);
      if (VEC && y_split) store_split4(y_split, n, off, o[0], o[1], o[2], o[3]);
    });
}

// (sum g1, sum g1 * xhat1, sum g2, sum g2 * xhat2) per (image, channel, row chunk) in one read of u and dy, written into the slab
// layout of bn_partial_kernel<1> over 2C channels, so that bn_bwd_final_kernel finishes it
template <bool VEC>
__global__ void __launch_bounds__(256) pair_blend_partial_kernel(const float* __restrict__ u, const float* __restrict__ dy,
                                                                 const float* __restrict__ label, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, float* __restrict__ part, int R, int C,
                                                                 int rows_per_chunk, int act, float slope, size_t bps) {
  const int b = blockIdx.z, C2 = 2 * C;
  const size_t bys = (size_t)R * C;
  u += (size_t)b * 2 * bys; dy += (size_t)b * bys; part += (size_t)b * bps;
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
  const int c = blockIdx.y * BN_CH + tx * 4;
  const int nv = min(4, C - c);                        // <= 0: this column of threads has no channel
  float s[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) s[q][j] = 0.f;
  if (c < C) {
    const float w2 = label[b], w1 = 1.f - w2;
    mean += (size_t)b * C2; rstd += (size_t)b * C2;
    const ChanConst s1 = chan_const(mean, rstd, nullptr, nullptr, c, nv);
    const ChanConst s2 = chan_const(mean, rstd, nullptr, nullptr, C + c, nv);
    const int r0 = blockIdx.x * rows_per_chunk;
    const int r1 = min(R, r0 + rows_per_chunk);
    auto accum = [&](const vp_f32x4& va, const vp_f32x4& vb, const vp_f32x4& d) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x1 = (va[j] - s1.mu[j]) * s1.rs[j], x2 = (vb[j] - s2.mu[j]) * s2.rs[j];
        const float g1 = pair_g(w1, d[j], pair_pre(va[j], s1.mu[j], s1.rs[j], 1), act, slope);
        const float g2 = pair_g(w2, d[j], pair_pre(vb[j], s2.mu[j], s2.rs[j], 1), act, slope);
        s[0][j] += g1;
        s[1][j] = fmaf(g1, x1, s[1][j]);
        s[2][j] += g2;
        s[3][j] = fmaf(g2, x2, s[3][j]);
      }
    };
    // NOT walk_rows: the compiler contracts `s += g` into an fma, or not, depending on the form of this loop (vector or scalar rows,
    // trip or tail), so any restatement moves last bits of the sums for the activations with a rounded derivative
    int r = r0 + ty;
    for (; r + 3 * BN_TY < r1; r += 4 * BN_TY) {
      vp_f32x4 va[4], vb[4], vd[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float* p = u + (size_t)(r + k * BN_TY) * C2 + c;
        va[k] = ld4(p, VEC, nv);
        vb[k] = ld4(p + C, VEC, nv);
        vd[k] = ld4(dy + (size_t)(r + k * BN_TY) * C + c, VEC, nv);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) accum(va[k], vb[k], vd[k]);
    }
    for (; r < r1; r += BN_TY) {
      const float* p = u + (size_t)r * C2 + c;
      accum(ld4(p, VEC, nv), ld4(p + C, VEC, nv), ld4(dy + (size_t)r * C + c, VEC, nv));
    }
  }
  const float t = block_colsum<4>(s);                                  // 4 sums x 64 channels = 256 threads
  const int q = threadIdx.x / BN_CH, cg = blockIdx.y * BN_CH + threadIdx.x % BN_CH;
  // q & 1: 0 = sum g, 1 = sum g * xhat (the two slabs of bn_partial_kernel); q >> 1: branch, at channel offset C
  if (cg < C) part[((size_t)(q & 1) * gridDim.x + blockIdx.x) * C2 + (q >> 1) * C + cg] = t;
}

// du_j = rstd_j * (g_j - (sum g_j + xhat_j * sum g_j xhat_j) / R)  (norm = 1)  |  g_j  (norm = 0), both halves in one pass
template <bool VEC>
__global__ void __launch_bounds__(256) pair_blend_bwd_kernel(const float* __restrict__ u, const float* __restrict__ dy,
                                                             const float* __restrict__ label, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ sum_g,
                                                             const float* __restrict__ sum_gx, float* __restrict__ du,
                                                             u16_t* __restrict__ du_split, int R, int C, int rows_per_chunk, float invR,
                                                             int norm, int act, float slope) {
  const int b = blockIdx.z, C2 = 2 * C;
  const size_t bys = (size_t)R * C;
  u += (size_t)b * 2 * bys; du += (size_t)b * 2 * bys; dy += (size_t)b * bys;
  const int tx = threadIdx.x % BN_TX, ty = threadIdx.x / BN_TX;
  const int c = blockIdx.y * BN_CH + tx * 4;
  if (c >= C) return;
  const int nv = min(4, C - c);
  const float w2 = label[b], w1 = 1.f - w2;
  mean += (size_t)b * C2; rstd += (size_t)b * C2;
  const ChanConst s1 = chan_const(mean, rstd, nullptr, nullptr, c, norm ? nv : 0);
  const ChanConst s2 = chan_const(mean, rstd, nullptr, nullptr, C + c, norm ? nv : 0);
  float k0[2][4], k1[2][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool ok = norm && j < nv;
    const size_t i1 = (size_t)b * C2 + c + j, i2 = i1 + C;
    k0[0][j] = ok ? sum_g[i1] * invR : 0.f; k1[0][j] = ok ? sum_gx[i1] * invR : 0.f;
    k0[1][j] = ok ? sum_g[i2] * invR : 0.f; k1[1][j] = ok ? sum_gx[i2] * invR : 0.f;
  }
  const size_t n = 2 * bys * gridDim.z;
  if (du_split) du_split += (size_t)b * 2 * bys;
  // bn=None without an activation (conv1, conv2 of the generator): du_j = w_j * dy, u is not read
  const bool need_u = norm || act != ACT_NONE;
  const int r0 = blockIdx.x * rows_per_chunk;
  const int r1 = min(R, r0 + rows_per_chunk);
  walk_rows<2>(r0 + ty, r1, true,                       // six independent loads in flight
    [&](int r) {
      const float* p = u + (size_t)r * C2 + c;
      Row<3> v = {};
      if (need_u) {
        ld4(v.v[0], p, VEC, nv);
        ld4(v.v[1], p + C, VEC, nv);
      }
      ld4(v.v[2], dy + (size_t)r * C + c, VEC, nv);
      return v;
    },
    [&](int r, const Row<3>& v) {
      vp_f32x4 oa, ob;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float g1 = pair_g(w1, v.v[2][j], pair_pre(v.v[0][j], s1.mu[j], s1.rs[j], norm), act, slope);
        const float g2 = pair_g(w2, v.v[2][j], pair_pre(v.v[1][j], s2.mu[j], s2.rs[j], norm), act, slope);
        if (norm) {
          const float x1 = (v.v[0][j] - s1.mu[j]) * s1.rs[j], x2 = (v.v[1][j] - s2.mu[j]) * s2.rs[j];
          oa[j] = bn_dx(s1.ga[j], s1.rs[j], g1, x1, k0[0][j], k1[0][j]);
          ob[j] = bn_dx(s2.ga[j], s2.rs[j], g2, x2, k0[1][j], k1[1][j]);
        } else {
          oa[j] = g1;
          ob[j] = g2;
        }
      }
      const size_t off = (size_t)r * C2 + c;
      st4(du + off, oa, VEC, nv);
      st4(du + off + C, ob, VEC, nv);
      if (VEC && du_split) {
        store_split4(du_split, n, off, oa[0], oa[1], oa[2], oa[3]);
        store_split4(du_split, n, off + C, ob[0], ob[1], ob[2], ob[3]);
      }
    });
}

// ---- host side: one workspace layout, one launcher per stage --------------------------------------------------------------------------
// Workspace of a B-image call over [R][C], in floats: the partial slabs part [B][2][chunks_r][C] at 0, then sum_g [B][C], sum_gx [B][C]
struct BnWs {
  BnGrid g;                         // the reduction grid the slabs are laid out for
  size_t bps;                       // partial floats per image
  size_t sum_g, sum_gx, floats;     // offsets of the two sums, and the size of it all
};
inline BnWs bn_ws(int B, int R, int C) {
  BnWs w;
  w.g = bn_grid(R, C);
  w.bps = (size_t)2 * w.g.chunks_r * C;
  w.sum_g = (size_t)B * w.bps;
  w.sum_gx = w.sum_g + (size_t)B * C;
  w.floats = w.sum_gx + (size_t)B * C;
  return w;
}
inline size_t bn_ws_bytes(int B, int R, int C) { return bn_ws(B, R, C).floats * sizeof(float); }

// check_launch for stage "partial" | "final" of the entry point `name`
static int check_stage(const char* name, const char* stage) {
  char what[96];
  snprintf(what, sizeof what, "%s(%s)", name, stage);
  return check_launch(what);
}

// All launchers: B images of [R][C] (B = 1: BatchNorm), `name` = the entry point, for error messages.
// Statistics: bn_partial_kernel<0> into the slabs, bn_stats_final_kernel into mean / rstd [B][C] (and the running statistics).
static int launch_stats(const char* name, const float* x, int B, int R, int C, float eps, float momentum, float* mean, float* rstd,
                        float* rm, float* rv, void* ws, hipStream_t s) {
  const BnWs w = bn_ws(B, R, C);
  const size_t bxs = (size_t)R * C;
  float* part = (float*)ws;
  hipLaunchKernelGGL((bn_partial_kernel<0>), dim3(w.g.chunks_r, w.g.chunks_c, B), dim3(256), 0, s, x, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, part, R, C,
                     w.g.rows_per_chunk, 0, 0.f, bxs, w.bps);
  int rc = check_stage(name, "partial");
  if (rc) return rc;
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3((C + FIN_C - 1) / FIN_C, 1, B), dim3(256), 0, s, (const float*)part, w.g.chunks_r, R, C,
                     eps, momentum, mean, rstd, rm, rv, x, w.bps, bxs);
  return check_stage(name, "final");
}

// Backward sums: partial(grid, part, bps) launches the kernel that fills the slabs over C channels, bn_bwd_final_kernel turns them into
// sum_g / sum_gx [B][C] inside the workspace (and dgamma / dbeta where given).
template <class Partial>
static int launch_bwd_sums(const char* name, int B, int R, int C, float* dgamma, float* dbeta, void* ws, hipStream_t s, Partial partial) {
  const BnWs w = bn_ws(B, R, C);
  float* part = (float*)ws;
  partial(w.g, part, w.bps);
  int rc = check_stage(name, "partial");
  if (rc) return rc;
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((C + FIN_C - 1) / FIN_C, 1, B), dim3(256), 0, s, (const float*)part, w.g.chunks_r, C,
                     part + w.sum_g, part + w.sum_gx, dgamma, dbeta, w.bps);
  return check_stage(name, "final");
}
static int launch_bn_bwd_sums(const char* name, const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                              const float* beta, float* dgamma, float* dbeta, int B, int R, int C, int act, float slope, void* ws,
                              hipStream_t s) {
  return launch_bwd_sums(name, B, R, C, dgamma, dbeta, ws, s, [&](const BnGrid& g, float* part, size_t bps) {
    hipLaunchKernelGGL((bn_partial_kernel<1>), dim3(g.chunks_r, g.chunks_c, B), dim3(256), 0, s, x, dy, mean, rstd, gamma, beta, part, R, C,
                       g.rows_per_chunk, act, slope, (size_t)R * C, bps);
  });
}

// Apply passes: the tiled kernel for C % 4 == 0, else the flat one (the callers have refused split planes there).  The caller checks
// the launch.
static void launch_apply_fwd(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* y,
                             void* y_split, int B, int R, int C, int act, float slope, int fmt, hipStream_t s, int ldy = 0) {
  const size_t bxs = (size_t)R * C;
  if (C % 4 == 0) {
    const BnGrid g = bn_apply_grid(R, C);
    hipLaunchKernelGGL(bn_act_fwd_tiled_kernel, dim3(g.chunks_r, g.chunks_c, B), dim3(256), 0, s, x, mean, rstd, gamma, beta, y,
                       (u16_t*)y_split, ldy ? ldy : C, R, C, g.rows_per_chunk, act, slope, bxs, fmt);
  } else {
    hipLaunchKernelGGL(bn_act_fwd_kernel, dim3(grid_for(bxs / 4 + 1, 256), 1, B), dim3(256), 0, s, x, mean, rstd, gamma, beta, y, bxs, C,
                       act, slope, bxs);
  }
}
static void launch_apply_bwd(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                             const float* sum_g, const float* sum_gx, float* dx, void* dx_split, int B, int R, int C, float invR, int act,
                             float slope, int fmt, float scale, int* sat, hipStream_t s) {
  const size_t bxs = (size_t)R * C;
  if (C % 4 == 0) {
    const BnGrid g = bn_apply_grid(R, C);
    hipLaunchKernelGGL(bn_act_bwd_tiled_kernel, dim3(g.chunks_r, g.chunks_c, B), dim3(256), 0, s, x, dy, mean, rstd, gamma, beta, sum_g,
                       sum_gx, dx, (u16_t*)dx_split, R, C, g.rows_per_chunk, invR, act, slope, bxs, fmt, scale, sat);
  } else {
    hipLaunchKernelGGL(bn_act_bwd_kernel, dim3(grid_for(bxs / 4 + 1, 256), 1, B), dim3(256), 0, s, x, dy, mean, rstd, gamma, beta, sum_g,
                       sum_gx, dx, bxs, C, invR, act, slope, bxs);
  }
}

}  // namespace vp

using namespace vp;

extern "C" {

size_t vp_bn_workspace_bytes(int R, int C) { return bn_ws_bytes(1, R, C); }

int vp_bn_stats_f32(const float* x, int R, int C, float eps, float momentum, float* mean, float* rstd, float* running_mean,
                    float* running_var, void* ws, size_t ws_bytes, vp_stream stream) {
  VP_REQUIRE(x && mean && rstd && ws && R > 0 && C > 0, "vp_bn_stats_f32: bad arguments");
  if (ws_bytes < vp_bn_workspace_bytes(R, C)) return fail(VP_ERR_WORKSPACE, "vp_bn_stats_f32: workspace too small");
  return launch_stats("vp_bn_stats_f32", x, 1, R, C, eps, momentum, mean, rstd, running_mean, running_var, ws, (hipStream_t)stream);
}

static int bn_act_fwd_impl(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* y,
                           void* y_split, int R, int C, int act, float slope, vp_stream stream, int fmt) {
  VP_REQUIRE(fmt == SPLIT_BF16 || fmt == SPLIT_F16, "vp_bn_act_fwd_split_fmt_f32: format 0 (bf16 pair) or 1 (fp16 pair)");
  VP_REQUIRE(x && mean && rstd && (y || y_split) && R > 0 && C > 0, "vp_bn_act_fwd: bad arguments");
  VP_REQUIRE(!y_split || C % 4 == 0, "vp_bn_act_fwd_split_f32: C must be a multiple of 4");
  launch_apply_fwd(x, mean, rstd, gamma, beta, y, y_split, 1, R, C, act, slope, fmt, (hipStream_t)stream);
  return check_launch("vp_bn_act_fwd");
}

int vp_bn_act_fwd_f32(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* y,
                      int R, int C, int act, float slope, vp_stream stream) {
  VP_REQUIRE(y, "vp_bn_act_fwd_f32: y is null");
  return bn_act_fwd_impl(x, mean, rstd, gamma, beta, y, nullptr, R, C, act, slope, stream, SPLIT_BF16);
}

int vp_bn_act_fwd_split_f32(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                            float* y, void* y_split, int R, int C, int act, float slope, vp_stream stream) {
  return bn_act_fwd_impl(x, mean, rstd, gamma, beta, y, y_split, R, C, act, slope, stream, SPLIT_BF16);
}

int vp_bn_act_fwd_split_fmt_f32(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                float* y, void* y_split, int R, int C, int act, float slope, int fmt, vp_stream stream) {
  return bn_act_fwd_impl(x, mean, rstd, gamma, beta, y, y_split, R, C, act, slope, stream, fmt);
}

static int bn_act_bwd_impl(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                           const float* beta, float* dx, void* dx_split, float* dgamma, float* dbeta, int R, int C, int act,
                           float slope, int batch_stats, void* ws, size_t ws_bytes, vp_stream stream, int fmt, float scale, int* sat) {
  VP_REQUIRE(x && dy && mean && rstd && (dx || dx_split) && ws && R > 0 && C > 0, "vp_bn_act_bwd_f32: bad arguments");
  VP_REQUIRE((fmt == SPLIT_BF16 || fmt == SPLIT_F16) && scale > 0.f, "vp_bn_act_bwd_split_fmt_f32: format 0 | 1, scale > 0");
  VP_REQUIRE(!dx_split || C % 4 == 0, "vp_bn_act_bwd_split_f32: C must be a multiple of 4");
  if (ws_bytes < vp_bn_workspace_bytes(R, C)) return fail(VP_ERR_WORKSPACE, "vp_bn_act_bwd_f32: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  int rc = launch_bn_bwd_sums("vp_bn_act_bwd_f32", x, dy, mean, rstd, gamma, beta, dgamma, dbeta, 1, R, C, act, slope, ws, s);
  if (rc) return rc;
  const BnWs w = bn_ws(1, R, C);
  launch_apply_bwd(x, dy, mean, rstd, gamma, beta, (const float*)ws + w.sum_g, (const float*)ws + w.sum_gx, dx, dx_split, 1, R, C,
                   batch_stats ? 1.f / (float)R : 0.f, act, slope, fmt, scale, sat, s);
  return check_launch("vp_bn_act_bwd_f32(apply)");
}

int vp_bn_act_bwd_f32(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                      const float* beta, float* dx, float* dgamma, float* dbeta, int R, int C, int act, float slope,
                      int batch_stats, void* ws, size_t ws_bytes, vp_stream stream) {
  VP_REQUIRE(dx, "vp_bn_act_bwd_f32: dx is null");
  return bn_act_bwd_impl(x, dy, mean, rstd, gamma, beta, dx, nullptr, dgamma, dbeta, R, C, act, slope, batch_stats, ws, ws_bytes, stream,
                         SPLIT_BF16, 1.f, nullptr);
}

int vp_bn_act_bwd_split_fmt_f32(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                                const float* beta, float* dx, void* dx_split, float* dgamma, float* dbeta, int R, int C, int act,
                                float slope, int batch_stats, int fmt, float scale, void* ws, size_t ws_bytes, vp_stream stream) {
  return bn_act_bwd_impl(x, dy, mean, rstd, gamma, beta, dx, dx_split, dgamma, dbeta, R, C, act, slope, batch_stats, ws, ws_bytes, stream,
                         fmt, scale, nullptr);
}

int vp_bn_act_bwd_split_fmt_sat_f32(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                                    const float* beta, float* dx, void* dx_split, float* dgamma, float* dbeta, int R, int C, int act,
                                    float slope, int batch_stats, int fmt, float scale, int* saturated, void* ws, size_t ws_bytes,
                                    vp_stream stream) {
  return bn_act_bwd_impl(x, dy, mean, rstd, gamma, beta, dx, dx_split, dgamma, dbeta, R, C, act, slope, batch_stats, ws, ws_bytes, stream,
                         fmt, scale, saturated);
}

int vp_bn_act_bwd_split_f32(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, float* dx, void* dx_split, float* dgamma, float* dbeta, int R, int C, int act,
                            float slope, int batch_stats, void* ws, size_t ws_bytes, vp_stream stream) {
  return bn_act_bwd_impl(x, dy, mean, rstd, gamma, beta, dx, dx_split, dgamma, dbeta, R, C, act, slope, batch_stats, ws, ws_bytes, stream,
                         SPLIT_BF16, 1.f, nullptr);
}

// ---- nn.InstanceNorm2d(affine=False) + activation: the same kernels with blockIdx.z = image (models/blocks.py:22) --------
size_t vp_instnorm_workspace_bytes(int B, int R, int C) { return bn_ws_bytes(B, R, C); }

static int instnorm_act_fwd_impl(const float* x, float* y, void* y_split, float* mean, float* rstd, int B, int R, int C, float eps, int act,
                                 float slope, void* ws, size_t ws_bytes, vp_stream stream, int ldy = 0) {
  VP_REQUIRE(x && y && mean && rstd && ws && B > 0 && R > 0 && C > 0, "vp_instnorm_act_fwd_f32: bad arguments");
  VP_REQUIRE(!y_split || C % 4 == 0, "vp_instnorm_act_fwd_split_f32: C must be a multiple of 4");
  VP_REQUIRE(!ldy || (C % 4 == 0 && ldy % 4 == 0 && ldy >= C && aligned16(y)),
             "vp_instnorm_act_fwd_ld_f32: C and ldy must be multiples of 4, ldy >= C, y 16-byte aligned");
  if (ws_bytes < vp_instnorm_workspace_bytes(B, R, C)) return fail(VP_ERR_WORKSPACE, "vp_instnorm_act_fwd_f32: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  int rc = launch_stats("vp_instnorm_act_fwd_f32", x, B, R, C, eps, 0.f, mean, rstd, nullptr, nullptr, ws, s);
  if (rc) return rc;
  launch_apply_fwd(x, mean, rstd, nullptr, nullptr, y, y_split, B, R, C, act, slope, SPLIT_BF16, s, ldy);
  return check_launch("vp_instnorm_act_fwd_f32(apply)");
}

int vp_instnorm_act_fwd_ld_f32(const float* x, float* y, int ldy, float* mean, float* rstd, int B, int R, int C, float eps, int act,
                               float slope, void* ws, size_t ws_bytes, vp_stream stream) {
  VP_REQUIRE(ldy > 0, "vp_instnorm_act_fwd_ld_f32: ldy must be positive");
  return instnorm_act_fwd_impl(x, y, nullptr, mean, rstd, B, R, C, eps, act, slope, ws, ws_bytes, stream, ldy);
}

int vp_instnorm_act_fwd_f32(const float* x, float* y, float* mean, float* rstd, int B, int R, int C, float eps, int act,
                            float slope, void* ws, size_t ws_bytes, vp_stream stream) {
  return instnorm_act_fwd_impl(x, y, nullptr, mean, rstd, B, R, C, eps, act, slope, ws, ws_bytes, stream);
}

int vp_instnorm_act_fwd_split_f32(const float* x, float* y, void* y_split, float* mean, float* rstd, int B, int R, int C, float eps,
                                  int act, float slope, void* ws, size_t ws_bytes, vp_stream stream) {
  VP_REQUIRE(y_split, "vp_instnorm_act_fwd_split_f32: null split output");
  return instnorm_act_fwd_impl(x, y, y_split, mean, rstd, B, R, C, eps, act, slope, ws, ws_bytes, stream);
}

static int instnorm_act_bwd_impl(const float* x, const float* dy, const float* mean, const float* rstd, float* dx, void* dx_split, int B,
                                 int R, int C, int act, float slope, void* ws, size_t ws_bytes, vp_stream stream) {
  VP_REQUIRE(x && dy && mean && rstd && dx && ws && B > 0 && R > 0 && C > 0, "vp_instnorm_act_bwd_f32: bad arguments");
  VP_REQUIRE(!dx_split || C % 4 == 0, "vp_instnorm_act_bwd_split_f32: C must be a multiple of 4");
  if (ws_bytes < vp_instnorm_workspace_bytes(B, R, C)) return fail(VP_ERR_WORKSPACE, "vp_instnorm_act_bwd_f32: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  int rc = launch_bn_bwd_sums("vp_instnorm_act_bwd_f32", x, dy, mean, rstd, nullptr, nullptr, nullptr, nullptr, B, R, C, act, slope, ws, s);
  if (rc) return rc;
  const BnWs w = bn_ws(B, R, C);
  launch_apply_bwd(x, dy, mean, rstd, nullptr, nullptr, (const float*)ws + w.sum_g, (const float*)ws + w.sum_gx, dx, dx_split, B, R, C,
                   1.f / (float)R, act, slope, SPLIT_BF16, 1.f, nullptr, s);
  return check_launch("vp_instnorm_act_bwd_f32(apply)");
}

int vp_instnorm_act_bwd_f32(const float* x, const float* dy, const float* mean, const float* rstd, float* dx, int B, int R, int C,
                            int act, float slope, void* ws, size_t ws_bytes, vp_stream stream) {
  return instnorm_act_bwd_impl(x, dy, mean, rstd, dx, nullptr, B, R, C, act, slope, ws, ws_bytes, stream);
}

int vp_instnorm_act_bwd_split_f32(const float* x, const float* dy, const float* mean, const float* rstd, float* dx, void* dx_split, int B,
                                  int R, int C, int act, float slope, void* ws, size_t ws_bytes, vp_stream stream) {
  VP_REQUIRE(dx_split, "vp_instnorm_act_bwd_split_f32: null split output");
  return instnorm_act_bwd_impl(x, dy, mean, rstd, dx, dx_split, B, R, C, act, slope, ws, ws_bytes, stream);
}

// ---- label-gated pair: InstanceNorm statistics over the 2C stacked channels, then one blend pass ---------------------------------
size_t vp_pair_blend_workspace_bytes(int B, int R, int C) { return bn_ws_bytes(B, R, 2 * C); }

int vp_pair_blend_fwd_f32(const float* u, const float* label, float* y, void* y_split, float* mean, float* rstd, int B, int R, int C,
                          int norm, float eps, int act, float slope, void* ws, size_t ws_bytes, vp_stream stream) {
  VP_REQUIRE(u && label && y && B > 0 && B <= 65535 && R > 0 && C > 0 && C <= (1 << 29), "vp_pair_blend_fwd_f32: bad arguments");
  VP_REQUIRE(!norm || (mean && rstd && ws), "vp_pair_blend_fwd_f32: norm = 1 needs mean, rstd and a workspace");
  VP_REQUIRE(!y_split || C % 4 == 0, "vp_pair_blend_fwd_f32: split planes need C to be a multiple of 4");
  hipStream_t s = (hipStream_t)stream;
  if (norm) {
    if (ws_bytes < vp_pair_blend_workspace_bytes(B, R, C)) return fail(VP_ERR_WORKSPACE, "vp_pair_blend_fwd_f32: workspace too small");
    int rc = launch_stats("vp_pair_blend_fwd_f32", u, B, R, 2 * C, eps, 0.f, mean, rstd, nullptr, nullptr, ws, s);
    if (rc) return rc;
  }
  const BnGrid ga = bn_apply_grid(R, C);
  const dim3 grid(ga.chunks_r, ga.chunks_c, B);
  if (C % 4 == 0)
    hipLaunchKernelGGL((pair_blend_fwd_kernel<true>), grid, dim3(256), 0, s, u, label, (const float*)mean, (const float*)rstd, y,
                       (u16_t*)y_split, R, C, ga.rows_per_chunk, norm ? 1 : 0, act, slope);
  else
    hipLaunchKernelGGL((pair_blend_fwd_kernel<false>), grid, dim3(256), 0, s, u, label, (const float*)mean, (const float*)rstd, y,
                       (u16_t*)nullptr, R, C, ga.rows_per_chunk, norm ? 1 : 0, act, slope);
  return check_launch("vp_pair_blend_fwd_f32(apply)");
}

int vp_pair_blend_bwd_f32(const float* u, const float* dy, const float* label, const float* mean, const float* rstd, float* du,
                          void* du_split, int B, int R, int C, int norm, int act, float slope, void* ws, size_t ws_bytes,
                          vp_stream stream) {
  VP_REQUIRE(u && dy && label && du && B > 0 && B <= 65535 && R > 0 && C > 0 && C <= (1 << 29), "vp_pair_blend_bwd_f32: bad arguments");
  VP_REQUIRE(!norm || (mean && rstd && ws), "vp_pair_blend_bwd_f32: norm = 1 needs mean, rstd and a workspace");
  VP_REQUIRE(!du_split || C % 4 == 0, "vp_pair_blend_bwd_f32: split planes need C to be a multiple of 4");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = C % 4 == 0;
  const float* sum_g = nullptr;
  const float* sum_gx = nullptr;
  if (norm) {
    if (ws_bytes < vp_pair_blend_workspace_bytes(B, R, C)) return fail(VP_ERR_WORKSPACE, "vp_pair_blend_bwd_f32: workspace too small");
    // row chunks and slab layout of the 2C-channel InstanceNorm backward; one block covers 64 channels of both branches
    int rc = launch_bwd_sums("vp_pair_blend_bwd_f32", B, R, 2 * C, nullptr, nullptr, ws, s, [&](const BnGrid& g, float* part, size_t bps) {
      const dim3 grid(g.chunks_r, (C + BN_CH - 1) / BN_CH, B);
      if (vec)
        hipLaunchKernelGGL((pair_blend_partial_kernel<true>), grid, dim3(256), 0, s, u, dy, label, mean, rstd, part, R, C, g.rows_per_chunk,
                           act, slope, bps);
      else
        hipLaunchKernelGGL((pair_blend_partial_kernel<false>), grid, dim3(256), 0, s, u, dy, label, mean, rstd, part, R, C, g.rows_per_chunk,
                           act, slope, bps);
    });
    if (rc) return rc;
    const BnWs w = bn_ws(B, R, 2 * C);
    sum_g = (const float*)ws + w.sum_g; sum_gx = (const float*)ws + w.sum_gx;
  }
  const BnGrid ga = bn_apply_grid(R, C);
  const dim3 grid(ga.chunks_r, ga.chunks_c, B);
  const float invR = 1.f / (float)R;
  if (vec)
    hipLaunchKernelGGL((pair_blend_bwd_kernel<true>), grid, dim3(256), 0, s, u, dy, label, mean, rstd, sum_g, sum_gx, du, (u16_t*)du_split, R,
                       C, ga.rows_per_chunk, invR, norm ? 1 : 0, act, slope);
  else
    hipLaunchKernelGGL((pair_blend_bwd_kernel<false>), grid, dim3(256), 0, s, u, dy, label, mean, rstd, sum_g, sum_gx, du, (u16_t*)nullptr, R,
                       C, ga.rows_per_chunk, invR, norm ? 1 : 0, act, slope);
  return check_launch("vp_pair_blend_bwd_f32(apply)");
}

int vp_bn_small_fwd_f32(const float* x, int R, int C, float eps, float momentum, const float* gamma, const float* beta, float* mean,
                        float* rstd, float* running_mean, float* running_var, float* y, int act, float slope, vp_stream stream) {
  VP_REQUIRE(x && mean && rstd && R > 0 && C > 0, "vp_bn_small_fwd_f32: bad arguments");
  VP_REQUIRE(R <= BN_SMALL_R && C % 4 == 0, "vp_bn_small_fwd_f32: at most 64 rows, C a multiple of 4 (use vp_bn_stats_f32 + vp_bn_act_fwd_f32)");
  hipLaunchKernelGGL(bn_small_fwd_kernel, dim3((C + BN_CH - 1) / BN_CH), dim3(256), 0, (hipStream_t)stream, x, R, C, eps, momentum, gamma, beta,
                     mean, rstd, running_mean, running_var, y, act, slope);
  return check_launch("vp_bn_small_fwd_f32");
}

int vp_bn_small_bwd_f32(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        float* dx, float* dgamma, float* dbeta, int R, int C, int act, float slope, int batch_stats, vp_stream stream) {
  VP_REQUIRE(x && dy && mean && rstd && dx && R > 0 && C > 0, "vp_bn_small_bwd_f32: bad arguments");
  VP_REQUIRE(R <= BN_SMALL_R && C % 4 == 0, "vp_bn_small_bwd_f32: at most 64 rows, C a multiple of 4 (use vp_bn_act_bwd_f32)");
  hipLaunchKernelGGL(bn_small_bwd_kernel, dim3((C + BN_CH - 1) / BN_CH), dim3(256), 0, (hipStream_t)stream, x, dy, mean, rstd, gamma, beta, dx,
                     dgamma, dbeta, R, C, batch_stats ? 1.f / (float)R : 0.f, act, slope);
  return check_launch("vp_bn_small_bwd_f32");
}

int vp_act_fwd_f32(const float* x, float* y, size_t n, int act, float slope, vp_stream stream) {
  VP_REQUIRE(x && y && n > 0, "vp_act_fwd_f32: bad arguments");
  hipLaunchKernelGGL(act_fwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, n, act, slope);
  return check_launch("vp_act_fwd_f32");
}

int vp_act_bwd_from_y_f32(const float* y, const float* dy, float* dx, size_t n, int act, float slope, vp_stream stream) {
  VP_REQUIRE(y && dy && dx && n > 0, "vp_act_bwd_from_y_f32: bad arguments");
  hipLaunchKernelGGL(act_bwd_from_y_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, y, dy, dx, n, act, slope);
  return check_launch("vp_act_bwd_from_y_f32");
}
}
