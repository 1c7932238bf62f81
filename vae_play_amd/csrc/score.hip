// Per-image scoring of a trained VAE (infer.FusedVAEInference.score): the reconstruction term per row, the reparameterisation
// with the log density ratio of the draw, and the K-sample importance-weighted bound.  fp32 VALU, wave64, no floating-point
// atomics: every sum has a fixed order, so two runs return the same bits.
//
// The terms are the reference's (KL: models/networks.py:270; per-pixel F.binary_cross_entropy(reduction="sum")), kept per image.
// The importance-weighted bound (Burda et al., "Importance Weighted Autoencoders", 2016) has no counterpart in the reference:
// new functionality.
#include "score.h"

namespace vp {

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
  VP_REQUIRE(score_chunks(n) <= 65535, "vp_bce_rows_f32: rows longer than 65535 x %d elements", SCORE_CHUNK);
  if (ws_bytes < vp_bce_rows_workspace_bytes(rows, n)) return fail(VP_ERR_WORKSPACE, "vp_bce_rows_f32: workspace too small");
  return bce_rows_launch<false>(p, t, nullptr, rows, n, out, nullptr, ws, (hipStream_t)stream, "vp_bce_rows_f32");
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
