// SelfAttentionBlock (models/blocks.py:68-96) without the N x N map: y = gamma softmax(Q K^T) V + x per image, forward and backward,
// exact fp32 on v_mfma_f32_16x16x4_f32 with fp32 accumulation.  Per image Q, K are (N, dq) and V, X, dO are (N, C), row-major: the
// NHWC memory of the block's maps.
//
// One structure serves all four matrix kernels.  A workgroup (4 waves) owns a STATIONARY tile of 64 rows, 16 per wave, and SWEEPS
// the other side of the attention map in tiles of 64 rows.  For a swept tile it forms T[y][x] = sum_k Y[y][k] X[x][k] with the swept
// row y on the MFMA's row index and its own row x on the lane, so the 16 results a lane holds (4 sub-tiles x 4 registers) are
// T[16 t + 4 (lane / 16) + reg][lane % 16].  That is already the A operand of the next product, out[x][c] += sum_y M[y][x] W[y][c]:
// k-step j of sub-tile t takes register j, the B operand is row 16 t + 4 (lane / 16) + j of the W tile in LDS.  Nothing crosses LDS
// between the two products, and a row statistic of x (the online softmax's max and sum, lse, delta) is one value per lane.
//   forward       x = query, y = key    M = exp(S - m) with running max / sum     W = V   out = O      channel chunk per workgroup
//   dV            x = key,   y = query  M = P = exp(S - lse[y])                   W = g   out = dV     channel chunk per workgroup
//   dK            x = key,   y = query  M = dS = P (gamma dP - delta[y])          W = Q   out = dK     dP summed over all of C
//   dQ            x = query, y = key    M = dS = P (gamma dP - delta[x])          W = K   out = dQ     dP summed over all of C
// Contractions (over dq for S, over C for dP) run in chunks of 32 columns staged through LDS, one chunk prefetched into registers
// while the previous one feeds the MFMAs; the padding of dq and C to the chunk is zeros written into LDS, never global memory.
// A lane reads its four k values of a 16-column block as one 16-byte LDS load; both operands permute k the same way, so the sum is
// complete.  Rows past N are staged as zeros; swept rows past N are masked (forward: energy -inf BEFORE the row max, since the
// block's q and k end in a ReLU and a phantom key of energy 0 would take real weight; backward: M = 0).
// No atomics and no hand-off between workgroups: every output element is written by exactly one lane, dgamma is reduced from
// per-workgroup partials in a fixed order.  Two runs give the same bits.
#include "attention.h"
#include <cmath>

namespace vp {
namespace {

using f4 = __attribute__((ext_vector_type(4))) float;

constexpr int TY = kAttnTile, DK = kAttnDK, LDK = DK + 4;      // LDS row stride of a staged chunk: 16-byte rows, banks spread

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// ---- a 64 x 32 chunk of a row-major matrix on its way to LDS: two runs of 4 consecutive columns per thread, each run one 16-byte
// load or (ld % 4 != 0, or an unaligned base) four 4-byte loads off the same address, so both paths share their address registers
__device__ __forceinline__ void load_run(float* r, const float* __restrict__ p, bool row_ok, int col, int ncols, bool vec) {
  if (vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row_ok && col < ncols) v = *reinterpret_cast<const float4*>(p);
    r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (row_ok && col + e < ncols) ? p[e] : 0.f;
  }
}
struct Stage {
  float r[8];
};
__device__ __forceinline__ void stage_load(Stage& s, const float* __restrict__ m, int ld, int row0, int nrows, int col0, int ncols, bool vec) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int idx = threadIdx.x + 256 * i, row = row0 + (idx >> 3), col = col0 + (idx & 7) * 4;
    load_run(s.r + 4 * i, m + row * ld + col, row < nrows, col, ncols, vec);
  }
}
__device__ __forceinline__ void stage_store(const Stage& s, float* lds) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int idx = threadIdx.x + 256 * i;
    *reinterpret_cast<float4*>(lds + (idx >> 3) * LDK + (idx & 7) * 4) = make_float4(s.r[4 * i], s.r[4 * i + 1], s.r[4 * i + 2], s.r[4 * i + 3]);
  }
}

// ---- the 64 x 16 NT tile W of the second product, NT runs per thread ----------------------------------------------------------------
template <int NT>
struct WStage {
  float r[4 * NT];
};
template <int NT>
__device__ __forceinline__ void wstage_load(WStage<NT>& s, const float* __restrict__ m, int ld, int row0, int nrows, int col0, int ncols, bool vec) {
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int idx = threadIdx.x + 256 * i, row = row0 + idx / (4 * NT), col = col0 + (idx % (4 * NT)) * 4;
    load_run(s.r + 4 * i, m + row * ld + col, row < nrows, col, ncols, vec);
  }
}
template <int NT>
__device__ __forceinline__ void wstage_store(const WStage<NT>& s, float* lds) {
  constexpr int LDW = 16 * NT + 4;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int idx = threadIdx.x + 256 * i;
    *reinterpret_cast<float4*>(lds + (idx / (4 * NT)) * LDW + (idx % (4 * NT)) * 4) =
        make_float4(s.r[4 * i], s.r[4 * i + 1], s.r[4 * i + 2], s.r[4 * i + 3]);
  }
}

// acc[t][reg] += sum over the chunk's 32 columns of Y[16 t + 4 g + reg][k] X[16 wave + r][k]      (r = lane % 16, g = lane / 16)
__device__ __forceinline__ void chunk_mma(f4 (&acc)[4], const float* sy, const float* sx, int wave, int r, int g) {
#pragma unroll
  for (int kb = 0; kb < DK / 16; ++kb) {
    const float4 b = *reinterpret_cast<const float4*>(sx + (16 * wave + r) * LDK + 16 * kb + 4 * g);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float4 a = *reinterpret_cast<const float4*>(sy + (16 * t + r) * LDK + 16 * kb + 4 * g);
      acc[t] = mfma4(a.x, b.x, acc[t]);
      acc[t] = mfma4(a.y, b.y, acc[t]);
      acc[t] = mfma4(a.z, b.z, acc[t]);
      acc[t] = mfma4(a.w, b.w, acc[t]);
    }
  }
}

// out[n][reg] += sum over the 64 swept rows of M[y][x = 16 wave + r] W[y][16 n + r]; out row = 16 wave + 4 g + reg
template <int NT>
__device__ __forceinline__ void second_mma(f4 (&out)[NT], const f4 (&mt)[4], const float* sw, int r, int g) {
  constexpr int LDW = 16 * NT + 4;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* row = sw + (16 * t + 4 * g + j) * LDW + r;
      const float a = mt[t][j];
#pragma unroll
      for (int n = 0; n < NT; ++n) out[n] = mfma4(a, row[16 * n], out[n]);
      __builtin_amdgcn_sched_barrier(0);      // keeps the 16 NT LDS reads from all being hoisted ahead of the MFMAs (registers)
    }
}

__device__ __forceinline__ float group_max(float v) {      // over the four lanes that share lane % 16
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// ---- forward (FWD) and dV (!FWD): one channel chunk of 16 NT columns per workgroup ---------------------------------------------------
//   FWD   xs = Q, ys = K, w = V;  writes o, y = gamma o + res, and lse from the workgroups of chunk 0
//  !FWD   xs = K, ys = Q, w = g;  reads lse; writes out_o = dV = gamma P^T g
template <int NT, bool FWD>
__global__ void __launch_bounds__(256, 3) attn_pv_kernel(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ w,
                                                      const float* __restrict__ res, const float* __restrict__ gamma,
                                                      const float* __restrict__ lse_in, float* __restrict__ out_y, float* __restrict__ out_o,
                                                      float* __restrict__ lse_out, int N, int dq, int C, int vec_s, int vec_c) {
  constexpr int CC = 16 * NT, LDW = CC + 4;
  __shared__ __attribute__((aligned(16))) float sx[TY * LDK];
  __shared__ __attribute__((aligned(16))) float sy[TY * LDK];
  __shared__ __attribute__((aligned(16))) float sw[TY * LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, x0 = blockIdx.x * TY, c0 = blockIdx.y * CC;
  const size_t is = (size_t)b * N * dq, ic = (size_t)b * N * C;
  const float* xsb = xs + is;
  const float* ysb = ys + is;
  const float* wb = w + ic;
  const int ns = (dq + DK - 1) / DK;
  float m = -INFINITY, l = 0.f;
  f4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f4{0.f, 0.f, 0.f, 0.f};
  Stage stx, sty;
  if (ns == 1) {      // the stationary operand fits one chunk: staged once, made visible by the first barrier of the sweep
    stage_load(stx, xsb, dq, x0, N, 0, dq, vec_s);
    stage_store(stx, sx);
  }
  for (int y0 = 0; y0 < N; y0 += TY) {
    WStage<NT> stw;
    wstage_load<NT>(stw, wb, C, y0, N, c0, C, vec_c);      // in flight under the first product
    float rl[16];
    if (!FWD) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int yy = y0 + 16 * (i >> 2) + 4 * g + (i & 3);
        rl[i] = yy < N ? lse_in[(size_t)b * N + yy] : 0.f;
      }
    }
    f4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) s[t] = f4{0.f, 0.f, 0.f, 0.f};
    stage_load(sty, ysb, dq, y0, N, 0, dq, vec_s);
    if (ns > 1) stage_load(stx, xsb, dq, x0, N, 0, dq, vec_s);
    for (int ch = 0; ch < ns; ++ch) {
      stage_store(sty, sy);
      if (ns > 1) stage_store(stx, sx);
      __syncthreads();
      if (ch + 1 < ns) {
        stage_load(sty, ysb, dq, y0, N, (ch + 1) * DK, dq, vec_s);
        stage_load(stx, xsb, dq, x0, N, (ch + 1) * DK, dq, vec_s);
      }
      chunk_mma(s, sy, sx, wave, r, g);
      __syncthreads();
    }
    // every wave is past the previous tile's second product (it sits before the barriers above), so sw is free
    wstage_store<NT>(stw, sw);
    if (FWD) {
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (y0 + 16 * t + 4 * g + j >= N) s[t][j] = -INFINITY;      // before the max: a phantom key must not count as energy 0
          mx = fmaxf(mx, s[t][j]);
        }
      const float mnew = fmaxf(m, group_max(mx));      // finite: every swept tile has at least one real key
      const float alpha = __expf(m - mnew);
      float sum = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s[t][j] = __expf(s[t][j] - mnew);
          sum += s[t][j];
        }
      l = l * alpha + group_sum(sum);
      m = mnew;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float a = __shfl(alpha, 4 * g + j, 64);      // the accumulators' rows are queries 4 g + j; their factor lives on that lane
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n][j] *= a;
      }
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[t][j] = (y0 + 16 * t + 4 * g + j < N) ? __expf(s[t][j] - rl[4 * t + j]) : 0.f;
    }
    __syncthreads();
    second_mma<NT>(acc, s, sw, r, g);
  }
  const float gam = gamma[0];
  if (FWD) {
    const float inv = 1.f / l;
    if (blockIdx.y == 0 && g == 0 && x0 + 16 * wave + r < N) lse_out[(size_t)b * N + x0 + 16 * wave + r] = m + logf(l);
    float ils[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ils[j] = __shfl(inv, 4 * g + j, 64);      // all 64 lanes take part, before any row is skipped
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float il = ils[j];
      const int row = x0 + 16 * wave + 4 * g + j;
      if (row >= N) continue;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int c = c0 + 16 * n + r;
        if (c >= C) continue;
        const size_t at = ic + (size_t)row * C + c;
        const float ov = acc[n][j] * il;
        out_o[at] = ov;
        out_y[at] = gam * ov + res[at];
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = x0 + 16 * wave + 4 * g + j;
      if (row >= N) continue;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int c = c0 + 16 * n + r;
        if (c < C) out_o[ic + (size_t)row * C + c] = gam * acc[n][j];
      }
    }
  }
}

// ---- dK (KS: keys stationary, queries swept) and dQ (!KS): dS needs dP over all of C, so the C contraction loops inside ---------------
//   KS   xs = K, xc = V, ys = Q, yc = g    out = dK = dS^T Q     lse, delta belong to the swept row
//  !KS   xs = Q, xc = g, ys = K, yc = V    out = dQ = dS K       lse, delta belong to the lane's own row
// One workgroup holds 16 NTD columns of dq (all of it up to dq = 128; beyond that blockIdx.y chunks the output columns).
template <int NTD, bool KS>
__global__ void __launch_bounds__(256, 2) attn_ds_kernel(const float* __restrict__ xs, const float* __restrict__ xc, const float* __restrict__ ys,
                                                      const float* __restrict__ yc, const float* __restrict__ lse,
                                                      const float* __restrict__ delta, const float* __restrict__ gamma,
                                                      float* __restrict__ out, int N, int dq, int C, int vec_s, int vec_c) {
  constexpr int DD = 16 * NTD, LDW = DD + 4;
  __shared__ __attribute__((aligned(16))) float sx[TY * LDK];
  __shared__ __attribute__((aligned(16))) float sy[TY * LDK];
  __shared__ __attribute__((aligned(16))) float sw[TY * LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, x0 = blockIdx.x * TY, d0 = blockIdx.y * DD;
  const size_t is = (size_t)b * N * dq, ic = (size_t)b * N * C, ir = (size_t)b * N;
  const float* xsb = xs + is;
  const float* ysb = ys + is;
  const float* xcb = xc + ic;
  const float* ycb = yc + ic;
  const int ns = (dq + DK - 1) / DK, total = ns + (C + DK - 1) / DK;
  const float gam = gamma[0];
  float lx = 0.f, dlx = 0.f;
  if (!KS && x0 + 16 * wave + r < N) {
    lx = lse[ir + x0 + 16 * wave + r];
    dlx = delta[ir + x0 + 16 * wave + r];
  }
  f4 acc[NTD];
#pragma unroll
  for (int n = 0; n < NTD; ++n) acc[n] = f4{0.f, 0.f, 0.f, 0.f};
  Stage stx, sty;
  auto load_chunk = [&](int i, int y0) {
    if (i < ns) {
      stage_load(sty, ysb, dq, y0, N, i * DK, dq, vec_s);
      stage_load(stx, xsb, dq, x0, N, i * DK, dq, vec_s);
    } else {
      stage_load(sty, ycb, C, y0, N, (i - ns) * DK, C, vec_c);
      stage_load(stx, xcb, C, x0, N, (i - ns) * DK, C, vec_c);
    }
  };
  for (int y0 = 0; y0 < N; y0 += TY) {
    WStage<NTD> stw;
    wstage_load<NTD>(stw, ysb, dq, y0, N, d0, dq, vec_s);
    float rl[16], rd[16];
    if (KS) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int yy = y0 + 16 * (i >> 2) + 4 * g + (i & 3);
        rl[i] = yy < N ? lse[ir + yy] : 0.f;
        rd[i] = yy < N ? delta[ir + yy] : 0.f;
      }
    }
    f4 s[4], dp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) s[t] = dp[t] = f4{0.f, 0.f, 0.f, 0.f};
    load_chunk(0, y0);
    for (int i = 0; i < total; ++i) {
      stage_store(sty, sy);
      stage_store(stx, sx);
      __syncthreads();
      if (i + 1 < total) load_chunk(i + 1, y0);
      if (i < ns) chunk_mma(s, sy, sx, wave, r, g);
      else chunk_mma(dp, sy, sx, wave, r, g);
      __syncthreads();
    }
    wstage_store<NTD>(stw, sw);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = __expf(s[t][j] - (KS ? rl[4 * t + j] : lx));
        const float ds = p * (gam * dp[t][j] - (KS ? rd[4 * t + j] : dlx));
        s[t][j] = (y0 + 16 * t + 4 * g + j < N) ? ds : 0.f;
      }
    __syncthreads();
    second_mma<NTD>(acc, s, sw, r, g);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = x0 + 16 * wave + 4 * g + j;
    if (row >= N) continue;
#pragma unroll
    for (int n = 0; n < NTD; ++n) {
      const int d = d0 + 16 * n + r;
      if (d < dq) out[is + (size_t)row * dq + d] = acc[n][j];
    }
  }
}

// ---- the row pass: delta[row] = gamma sum_c g o, and one partial of sum g o per workgroup -----------------------------------------------
__global__ void __launch_bounds__(256) attn_delta_kernel(const float* __restrict__ gr, const float* __restrict__ o, const float* __restrict__ gamma,
                                                         float* __restrict__ delta, float* __restrict__ partial, size_t rows, int C) {
  __shared__ float sh[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float gam = gamma[0];
  float tot = 0.f;
  for (size_t row = (size_t)blockIdx.x * 4 + wave; row < rows; row += (size_t)gridDim.x * 4) {
    const float* a = gr + row * C;
    const float* c = o + row * C;
    float v = 0.f;
    for (int i = lane; i < C; i += 64) v += a[i] * c[i];
    v = wave_sum(v);
    if (lane == 0) delta[row] = gam * v;
    tot += v;
  }
  if (lane == 0) sh[wave] = tot;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ void __launch_bounds__(256) attn_dgamma_kernel(const float* __restrict__ partial, int n, float* __restrict__ dgamma) {
  __shared__ float sh[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += partial[i];
  const float t = block_sum4(a, sh);
  if (threadIdx.x == 0) dgamma[0] = t;
}

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" int vp_attn_fwd_f32(const float* q, const float* k, const float* v, const float* x, const float* gamma, float* y, float* o,
                               float* lse, int B, int N, int dq, int C, vp_stream stream) {
  if (int rc = attn_check_dims("vp_attn_fwd_f32", B, N, dq, C)) return rc;
  VP_REQUIRE(q && k && v && x && gamma && y && o && lse, "vp_attn_fwd_f32: null pointer");
  const AttnPlan pl = attn_plan(B, N, dq, C);
  hipStream_t s = (hipStream_t)stream;
  const int vec_s = dq % 4 == 0 && aligned16(q, k), vec_c = C % 4 == 0 && aligned16(v);
  const dim3 grid(pl.tiles, pl.cchunks, B), blk(256);
  const float* none = nullptr;
  if (pl.nt_c == 4)
    hipLaunchKernelGGL((attn_pv_kernel<4, true>), grid, blk, 0, s, q, k, v, x, gamma, none, y, o, lse, N, dq, C, vec_s, vec_c);
  else
    hipLaunchKernelGGL((attn_pv_kernel<8, true>), grid, blk, 0, s, q, k, v, x, gamma, none, y, o, lse, N, dq, C, vec_s, vec_c);
  return check_launch("vp_attn_fwd_f32");
}

extern "C" size_t vp_attn_bwd_workspace_bytes(int B, int N, int dq, int C) {
  if (B <= 0 || N <= 0 || dq <= 0 || C <= 0) return 0;
  return attn_plan(B, N, dq, C).ws_floats * sizeof(float);
}

extern "C" int vp_attn_bwd_f32(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* g,
                               const float* gamma, float* dq_out, float* dk_out, float* dv_out, float* dgamma, void* ws, size_t ws_bytes,
                               int B, int N, int dq, int C, vp_stream stream) {
  if (int rc = attn_check_dims("vp_attn_bwd_f32", B, N, dq, C)) return rc;
  VP_REQUIRE(q && k && v && o && lse && g && gamma && dgamma && ws, "vp_attn_bwd_f32: null pointer");
  const AttnPlan pl = attn_plan(B, N, dq, C);
  if (ws_bytes < pl.ws_floats * sizeof(float))
    return fail(VP_ERR_WORKSPACE, "vp_attn_bwd_f32: workspace of %zu bytes, %zu needed", ws_bytes, pl.ws_floats * sizeof(float));
  hipStream_t s = (hipStream_t)stream;
  float* delta = (float*)ws + pl.ws_delta;
  float* partial = (float*)ws + pl.ws_partial;
  const int vec_s = dq % 4 == 0 && aligned16(q, k), vec_c = C % 4 == 0 && aligned16(v, g);
  const dim3 blk(256);
  hipLaunchKernelGGL(attn_delta_kernel, dim3(pl.row_blocks), blk, 0, s, g, o, gamma, delta, partial, (size_t)B * N, C);
  hipLaunchKernelGGL(attn_dgamma_kernel, dim3(1), blk, 0, s, (const float*)partial, pl.row_blocks, dgamma);
  const float* none = nullptr;
  float* nof = nullptr;
  if (dv_out) {
    const dim3 grid(pl.tiles, pl.cchunks, B);
    if (pl.nt_c == 4)
      hipLaunchKernelGGL((attn_pv_kernel<4, false>), grid, blk, 0, s, k, q, g, none, gamma, lse, nof, dv_out, nof, N, dq, C, vec_s, vec_c);
    else
      hipLaunchKernelGGL((attn_pv_kernel<8, false>), grid, blk, 0, s, k, q, g, none, gamma, lse, nof, dv_out, nof, N, dq, C, vec_s, vec_c);
  }
  const dim3 gridd(pl.tiles, pl.dchunks, B);
  const float* cdelta = delta;
  if (dk_out) {
    if (pl.nt_d == 2)
      hipLaunchKernelGGL((attn_ds_kernel<2, true>), gridd, blk, 0, s, k, v, q, g, lse, cdelta, gamma, dk_out, N, dq, C, vec_s, vec_c);
    else
      hipLaunchKernelGGL((attn_ds_kernel<8, true>), gridd, blk, 0, s, k, v, q, g, lse, cdelta, gamma, dk_out, N, dq, C, vec_s, vec_c);
  }
  if (dq_out) {
    if (pl.nt_d == 2)
      hipLaunchKernelGGL((attn_ds_kernel<2, false>), gridd, blk, 0, s, q, g, k, v, lse, cdelta, gamma, dq_out, N, dq, C, vec_s, vec_c);
    else
      hipLaunchKernelGGL((attn_ds_kernel<8, false>), gridd, blk, 0, s, q, g, k, v, lse, cdelta, gamma, dq_out, N, dq, C, vec_s, vec_c);
  }
  return check_launch("vp_attn_bwd_f32");
}
