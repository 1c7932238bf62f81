// The per-row BCE walk shared by score.hip (vp_bce_rows_f32) and project.hip (vp_bce_masked_rows_bwd_f32): one statement of the
// chunking, of which lane sums which element and of the reduction order, so that the two entry points return the same bits where
// they compute the same thing.  fp32 VALU, wave64, no floating-point atomics.
#pragma once
#include <stdint.h>
#include "common.h"
#include "problems.h"

namespace vp {

// elements of a row per workgroup: 256 lanes x 4 x 16 bytes.  A multiple of 4, so every chunk of a row starts at the row's own
// offset from a 16-byte boundary.
constexpr int SCORE_CHUNK = 4096;

inline int score_chunks(int n) { return (n + SCORE_CHUNK - 1) / SCORE_CHUNK; }

// grid (rows, chunks): workgroup (r, c) sums elements [c * SCORE_CHUNK, min(n, (c + 1) * SCORE_CHUNK)) of row r into
// dst[r * nchunk + c].  Where p and t sit at the same offset from a 16-byte boundary the chunk is read as up to 3 scalar head
// elements, 16-byte loads, and up to 3 scalar tail elements; else element by element (still coalesced).  Lane partials in
// fp32, the wave tree and the 4-wave sum in a fixed order.
// GRAD: every term is weighted by mask (NULL: all ones) and dlogit = mask * (p - t) is written in the same pass.  Which lane takes
// which element depends on p and t alone, as without GRAD; mask and dlogit move 16 bytes at a time where they share that offset
// and element by element where they do not.
template <bool GRAD>
static __global__ void __launch_bounds__(256) bce_rows_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                              const float* __restrict__ mask, int n, int nchunk,
                                                              float* __restrict__ dst, float* __restrict__ dlogit) {
  __shared__ float sh[4];
  const int r = blockIdx.x, c = blockIdx.y;
  const long long c0 = (long long)c * SCORE_CHUNK;
  const int len = (int)((long long)n - c0 < SCORE_CHUNK ? (long long)n - c0 : SCORE_CHUNK);
  const float* pr = p + (size_t)r * n + c0;
  const float* tr = t + (size_t)r * n + c0;
  const float* mr = GRAD && mask ? mask + (size_t)r * n + c0 : nullptr;
  float* dr = GRAD ? dlogit + (size_t)r * n + c0 : nullptr;
  const bool vec = (((uintptr_t)pr ^ (uintptr_t)tr) & 15) == 0;
  const bool mvec = (((uintptr_t)pr ^ (uintptr_t)mr) & 15) == 0, dvec = (((uintptr_t)pr ^ (uintptr_t)dr) & 15) == 0;
  const int to_boundary = (int)(((16 - ((uintptr_t)pr & 15)) & 15) >> 2);
  const int head = vec ? (to_boundary < len ? to_boundary : len) : len;
  float acc = 0.f;
  auto one = [&](int i) {
    if (GRAD) {
      const float m = mr ? mr[i] : 1.f;
      acc -= m * bce_term(pr[i], tr[i]);
      dr[i] = m * (pr[i] - tr[i]);
    } else {
      acc -= bce_term(pr[i], tr[i]);
    }
  };
  for (int i = threadIdx.x; i < head; i += 256) one(i);
  const int n4 = (len - head) >> 2;
  for (int i = threadIdx.x; i < n4; i += 256) {
    const int e = head + 4 * i;
    const vp_f32x4 pv = *reinterpret_cast<const vp_f32x4*>(pr + e);
    const vp_f32x4 tv = *reinterpret_cast<const vp_f32x4*>(tr + e);
    if (GRAD) {
      vp_f32x4 mv = {1.f, 1.f, 1.f, 1.f}, dv;
      if (mr) {
        if (mvec) mv = *reinterpret_cast<const vp_f32x4*>(mr + e);
        else
#pragma unroll
          for (int j = 0; j < 4; ++j) mv[j] = mr[e + j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc -= mv[j] * bce_term(pv[j], tv[j]);
        dv[j] = mv[j] * (pv[j] - tv[j]);
      }
      if (dvec) *reinterpret_cast<vp_f32x4*>(dr + e) = dv;
      else
#pragma unroll
        for (int j = 0; j < 4; ++j) dr[e + j] = dv[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc -= bce_term(pv[j], tv[j]);
    }
  }
  for (int i = head + 4 * n4 + threadIdx.x; i < len; i += 256) one(i);
  acc = block_sum4(acc, sh);
  if (threadIdx.x == 0) dst[(size_t)r * nchunk + c] = acc;
}

// one wavefront per row: the chunk partials in fp64, lanes stride the chunks, fixed-order tree
static __global__ void __launch_bounds__(64) bce_rows_final_kernel(const float* __restrict__ part, int nchunk, float* __restrict__ out) {
  const size_t base = (size_t)blockIdx.x * nchunk;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nchunk; i += 64) acc += (double)part[base + i];
  acc = wave_sum_d(acc);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)acc;
}

// the two stages: a row of one chunk is done by its workgroup; longer rows take the second, fixed-order stage
template <bool GRAD>
inline int bce_rows_launch(const float* p, const float* t, const float* mask, int rows, int n, float* out, float* dlogit, void* ws,
                           hipStream_t s, const char* what) {
  const int nchunk = score_chunks(n);
  hipLaunchKernelGGL(bce_rows_kernel<GRAD>, dim3(rows, nchunk), dim3(256), 0, s, p, t, mask, n, nchunk, nchunk == 1 ? out : (float*)ws,
                     dlogit);
  int rc = check_launch(what);
  if (rc || nchunk == 1) return rc;
  hipLaunchKernelGGL(bce_rows_final_kernel, dim3(rows), dim3(64), 0, s, (const float*)ws, nchunk, out);
  return check_launch(what);
}

}  // namespace vp
