// Per-image scoring of a trained VAE (infer.FusedVAEInference.score): the reconstruction term per row, the reparameterisation
// with the log density ratio of the draw, and the K-sample importance-weighted bound.  fp32 VALU, wave64, no floating-point
// atomics: every sum has a fixed order, so two runs return the same bits.
//
// The terms are the reference's (KL: models/networks.py:270; per-pixel F.binary_cross_entropy(reduction="sum")), kept per image.
// The importance-weighted bound (Burda et al., "Importance Weighted Autoencoders", 2016) has no counterpart in the reference:
// new functionality.
#include <stdint.h>
#include "common.h"
#include "problems.h"

namespace vp {

// elements of a row per workgroup: 256 lanes x 4 x 16 bytes.  A multiple of 4, so every chunk of a row starts at the row's own
// offset from a 16-byte boundary.
constexpr int SCORE_CHUNK = 4096;

inline int score_chunks(int n) { return (n + SCORE_CHUNK - 1) / SCORE_CHUNK; }

// the BCE term of reduce_partial_kernel<0> (elementwise.hip), the same expression and clamp
__device__ __forceinline__ float bce_term(float p, float t) {
  const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(logf(1.f - p), -100.f);
  return t * lp + (1.f - t) * lq;
}

// grid (rows, chunks): workgroup (r, c) sums elements [c * SCORE_CHUNK, min(n, (c + 1) * SCORE_CHUNK)) of row r into
// dst[r * nchunk + c].  Where p and t sit at the same offset from a 16-byte boundary the chunk is read as up to 3 scalar head
// elements, 16-byte loads, and up to 3 scalar tail elements; else element by element (still coalesced).  Lane partials in
// fp32, the wave tree and the 4-wave sum in a fixed order.
__global__ void __launch_bounds__(256) bce_rows_kernel(const float* __restrict__ p, const float* __restrict__ t, int n, int nchunk,
                                                       float* __restrict__ dst) {
  __shared__ float sh[4];
  const int r = blockIdx.x, c = blockIdx.y;
  const long long c0 = (long long)c * SCORE_CHUNK;
  const int len = (int)((long long)n - c0 < SCORE_CHUNK ? (long long)n - c0 : SCORE_CHUNK);
  const float* pr = p + (size_t)r * n + c0;
  const float* tr = t + (size_t)r * n + c0;
  const bool vec = (((uintptr_t)pr ^ (uintptr_t)tr) & 15) == 0;
  const int to_boundary = (int)(((16 - ((uintptr_t)pr & 15)) & 15) >> 2);
  const int head = vec ? (to_boundary < len ? to_boundary : len) : len;
  float acc = 0.f;
  for (int i = threadIdx.x; i < head; i += 256) acc -= bce_term(pr[i], tr[i]);
  const int n4 = (len - head) >> 2;
  for (int i = threadIdx.x; i < n4; i += 256) {
    const vp_f32x4 pv = *reinterpret_cast<const vp_f32x4*>(pr + head + 4 * i);
    const vp_f32x4 tv = *reinterpret_cast<const vp_f32x4*>(tr + head + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc -= bce_term(pv[j], tv[j]);
  }
  for (int i = head + 4 * n4 + threadIdx.x; i < len; i += 256) acc -= bce_term(pr[i], tr[i]);
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) dst[(size_t)r * nchunk + c] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// one wavefront per row: the chunk partials in fp64, lanes stride the chunks, fixed-order tree
__global__ void __launch_bounds__(64) bce_rows_final_kernel(const float* __restrict__ part, int nchunk, float* __restrict__ out) {
  const size_t base = (size_t)blockIdx.x * nchunk;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nchunk; i += 64) acc += (double)part[base + i];
  acc = wave_sum_d(acc);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)acc;
}

// one wavefront per sample, as latent_fwd_kernel (elementwise.hip) and with its expressions for z and kl in its order -- the two
// kernels write the same bits -- plus lr[b] = log p(z_b) - log q(z_b | x_b) = -1/2 sum_j z_j^2 + 1/2 sum_j (eps_j^2 + logvar_j)
// (z - mu = eps exp(logvar / 2); the 2 pi terms cancel)
__global__ void __launch_bounds__(64) latent_iw_fwd_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                           const float* __restrict__ eps, float* __restrict__ z, float* __restrict__ kl,
                                                           float* __restrict__ lr, int Z) {
  const int b = blockIdx.x;
  float acc = 0.f, sz = 0.f, sq = 0.f;
  for (int j = threadIdx.x; j < Z; j += 64) {
    const size_t i = (size_t)b * Z + j;
    const float m = mu[i], l = lv[i], e = eps[i];
    const float zv = e * expf(0.5f * l) + m;
    z[i] = zv;
    acc += -expf(l) - m * m + l + 1.f;
    sz += zv * zv;
    sq += e * e + l;
  }
  acc = wave_sum(acc);
  sz = wave_sum(sz);
  sq = wave_sum(sq);
  if (threadIdx.x == 0) {
    if (kl) kl[b] = -0.5f * acc;
    lr[b] = 0.5f * sq - 0.5f * sz;
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// one wavefront per image, lanes stride the K draws: logw = lr - nbce, then log-mean-exp with the row maximum subtracted first
// (the values are -1e3 .. -1e5: exp underflows otherwise).  K = 1: exp(0) = 1 and log 1 - log 1 = 0, the result IS logw[b][0];
// K equal values: the sum is K exactly and the two logarithms cancel.
__global__ void __launch_bounds__(64) iw_bound_kernel(const float* __restrict__ nbce, const float* __restrict__ lr, int K,
                                                      float* __restrict__ logw, float* __restrict__ iwae) {
  const size_t base = (size_t)blockIdx.x * K;
  float m = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 64) {
    const float w = lr[base + k] - nbce[base + k];
    if (logw) logw[base + k] = w;
    m = fmaxf(m, w);
  }
  m = wave_max(m);
  float s = 0.f;
  for (int k = threadIdx.x; k < K; k += 64) s += expf((lr[base + k] - nbce[base + k]) - m);
  s = wave_sum(s);
  if (threadIdx.x == 0) iwae[blockIdx.x] = m + (logf(s) - logf((float)K));
}

}  // namespace vp

using namespace vp;

extern "C" {

size_t vp_bce_rows_workspace_bytes(int rows, int n) {
  if (rows <= 0 || n <= 0) return 0;
  return (size_t)rows * score_chunks(n) * sizeof(float);
}

int vp_bce_rows_f32(const float* p, const float* t, int rows, int n, float* out, void* ws, size_t ws_bytes, vp_stream stream) {
  VP_REQUIRE(p && t && out && ws && rows > 0 && n > 0, "vp_bce_rows_f32: bad arguments");
  const int nchunk = score_chunks(n);
  VP_REQUIRE(nchunk <= 65535, "vp_bce_rows_f32: rows longer than 65535 x %d elements", SCORE_CHUNK);
  if (ws_bytes < vp_bce_rows_workspace_bytes(rows, n)) return fail(VP_ERR_WORKSPACE, "vp_bce_rows_f32: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  // a row of one chunk is done by its workgroup; longer rows take the second, fixed-order stage
  hipLaunchKernelGGL(bce_rows_kernel, dim3(rows, nchunk), dim3(256), 0, s, p, t, n, nchunk, nchunk == 1 ? out : (float*)ws);
  int rc = check_launch("vp_bce_rows_f32(partial)");
  if (rc || nchunk == 1) return rc;
  hipLaunchKernelGGL(bce_rows_final_kernel, dim3(rows), dim3(64), 0, s, (const float*)ws, nchunk, out);
  return check_launch("vp_bce_rows_f32(final)");
}

int vp_latent_iw_fwd_f32(const float* mu, const float* logvar, const float* eps, float* z, float* kl, float* lr, int B, int Z,
                         vp_stream stream) {
  VP_REQUIRE(mu && logvar && eps && z && lr && B > 0 && Z > 0, "vp_latent_iw_fwd_f32: bad arguments");
  hipLaunchKernelGGL(latent_iw_fwd_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, mu, logvar, eps, z, kl, lr, Z);
  return check_launch("vp_latent_iw_fwd_f32");
}

int vp_iw_bound_f32(const float* nbce, const float* lr, int B, int K, float* logw, float* iwae, vp_stream stream) {
  VP_REQUIRE(nbce && lr && iwae && B > 0 && K > 0, "vp_iw_bound_f32: bad arguments");
  hipLaunchKernelGGL(iw_bound_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, nbce, lr, K, logw, iwae);
  return check_launch("vp_iw_bound_f32");
}

}  // extern "C"
