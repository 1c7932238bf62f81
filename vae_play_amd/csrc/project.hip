// Latent projection of a trained VAE decoder (infer.FusedVAEInference.project / decode_grad): the gradient of the per-image
// reconstruction term with respect to z through the frozen eval-mode decoder, and the latent update.  Three kernels are new here;
// the input-gradient convolutions and the dense input gradient are the training plans'.  fp32 VALU, wave64, no floating-point
// atomics: every sum has a fixed order, so two runs return the same bits.
//
// Projection (searching the latent space for the z whose decode explains a given, possibly masked, image) has no counterpart in
// the reference: new functionality.  Its objective is the reference's per-pixel F.binary_cross_entropy(reduction="sum"), kept
// per image, plus a Gaussian prior on z.
#include "optim.h"
#include "score.h"
#include "split.h"

namespace vp {

// ---- backward of a folded block, from its OUTPUT -----------------------------------------------------------------------------------
// An eval-mode block computes u = relu(s c + t) per channel (s, t: the folded BatchNorm) and keeps u alone.  u > 0 exactly where the
// pre-activation is > 0, so   dc = dy * s * (u > 0).   u is fp32 or split bf16 planes (the mask is "hi + lo > 0": what the next
// layer read); dx is written as fp32 and / or as the split planes vp_split_f32 makes of that fp32 value.  The product is formed as
// (dy * s) * {1, 0}: a masked element is a zero with the sign of dy * s, as the same expression gives on fp32 tensors.
__device__ __forceinline__ float unsplit_bf16(u16_t hi, u16_t lo) {
  return __builtin_bit_cast(float, (uint32_t)hi << 16) + __builtin_bit_cast(float, (uint32_t)lo << 16);
}

// 16-byte form: n % 4 == 0, C % 4 == 0, every pointer 16-byte aligned.  A quad never crosses a row (C % 4 == 0).  dx may alias dy:
// a thread reads its quad before it writes it, and no other thread touches it.
__global__ void __launch_bounds__(256) affine_relu_bwd_kernel4(const float* dy, const float* __restrict__ u, const u16_t* __restrict__ us,
                                                               const float* __restrict__ scale, float* dx, u16_t* __restrict__ dxs,
                                                               size_t n, int C) {
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i * 4;
    const vp_f32x4 g = *reinterpret_cast<const vp_f32x4*>(dy + e);
    const vp_f32x4 s = *reinterpret_cast<const vp_f32x4*>(scale + e % C);
    vp_f32x4 uv;
    if (u) {
      uv = *reinterpret_cast<const vp_f32x4*>(u + e);
    } else {
      const u16x4_t h = *reinterpret_cast<const u16x4_t*>(us + e), l = *reinterpret_cast<const u16x4_t*>(us + n + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) uv[j] = unsplit_bf16(h[j], l[j]);
    }
    vp_f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (g[j] * s[j]) * (uv[j] > 0.f ? 1.f : 0.f);
    if (dx) *reinterpret_cast<vp_f32x4*>(dx + e) = o;
    if (dxs) store_split4(dxs, n, e, o[0], o[1], o[2], o[3]);
  }
}

// element by element: any C, any alignment
__global__ void __launch_bounds__(256) affine_relu_bwd_kernel1(const float* dy, const float* __restrict__ u, const u16_t* __restrict__ us,
                                                               const float* __restrict__ scale, float* dx, u16_t* __restrict__ dxs,
                                                               size_t n, int C) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float uv = u ? u[i] : unsplit_bf16(us[i], us[n + i]);
    const float o = (dy[i] * scale[i % C]) * (uv > 0.f ? 1.f : 0.f);
    if (dx) dx[i] = o;
    if (dxs) {
      u16_t h, l;
      split_f32(o, h, l);
      dxs[i] = h;
      dxs[n + i] = l;
    }
  }
}

// ---- one Adam step on the latents ------------------------------------------------------------------------------------------------
// adam_update (optim.h) on element i of z, in the form of v that adam_kernel (optim.hip: vp_adam_f32) applies to element i of a
// flat array of rows * Z elements below its streaming loop's threshold: ADAM_V_FMA_DECAY for an element of a whole 16-byte quad
// (i < n & ~3), ADAM_V_TWO_PRODUCTS for the last n & 3.  With prior_weight = 0 the two kernels write the same bits;
// tests/test_gpu_project_kernels.py holds them to each other.
//
// One wavefront per row of z [rows][Z], lanes stride the row.  Gradient g + prior_weight z (one fma).  The bias corrections are
// computed here from the step count READ FROM DEVICE MEMORY: count[0] = steps taken so far, this launch is step count[0] + 1.
// Nothing in this launch writes the counter -- latent_step_advance_kernel, a one-thread launch that follows it on the stream,
// does -- so every wavefront reads the same value.  prior[r] = prior_weight/2 |z_r|^2 of the z it READ (fixed-order wave tree).
// g == NULL: no update, prior alone.
__global__ void __launch_bounds__(64) latent_adam_kernel(float* __restrict__ z, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, const int* __restrict__ count, int Z, float lr,
                                                         float beta1, float beta2, float eps, float prior_weight,
                                                         float* __restrict__ prior) {
  const size_t base = (size_t)blockIdx.x * Z;
  const size_t quads_end = ((size_t)gridDim.x * Z) & ~(size_t)3;
  AdamStep k = {};
  if (g) k = adam_step_constants(lr, beta1, beta2, eps, count[0] + 1);
  float sq = 0.f;
  for (int j = threadIdx.x; j < Z; j += 64) {
    const size_t i = base + j;
    float zv = z[i];
    sq += zv * zv;
    if (g) {
      float mv = m[i], vv = v[i];
      adam_update(zv, fmaf(prior_weight, zv, g[i]), mv, vv, i < quads_end ? ADAM_V_FMA_DECAY : ADAM_V_TWO_PRODUCTS, 1.f, k);
      z[i] = zv;
      m[i] = mv;
      v[i] = vv;
    }
  }
  if (prior) {
    sq = wave_sum(sq);
    if (threadIdx.x == 0) prior[blockIdx.x] = prior_weight * (0.5f * sq);
  }
}

__global__ void latent_step_advance_kernel(int* count) { count[0] += 1; }

}  // namespace vp

using namespace vp;

extern "C" {

int vp_affine_relu_bwd_f32(const float* dy, const float* u, const void* u_split, const float* scale, float* dx, void* dx_split,
                           size_t R, int C, vp_stream stream) {
  VP_REQUIRE(dy && scale && R > 0 && C > 0, "vp_affine_relu_bwd_f32: bad arguments");
  VP_REQUIRE((u != nullptr) != (u_split != nullptr), "vp_affine_relu_bwd_f32: the output is given as fp32 or as split planes, one of the two");
  VP_REQUIRE(dx || dx_split, "vp_affine_relu_bwd_f32: no output");
  const size_t n = R * (size_t)C;
  const u16_t* us = (const u16_t*)u_split;
  u16_t* dxs = (u16_t*)dx_split;
  hipStream_t s = (hipStream_t)stream;
  // (the lo planes start n elements after the hi planes: 8-byte aligned with them when n % 4 == 0)
  if (C % 4 == 0 && aligned16(dy, u, scale, dx) && (((uintptr_t)us | (uintptr_t)dxs) & 7) == 0)
    hipLaunchKernelGGL(affine_relu_bwd_kernel4, dim3(grid_for(n / 4, 256, 256 * 16)), dim3(256), 0, s, dy, u, us, scale, dx, dxs, n, C);
  else
    hipLaunchKernelGGL(affine_relu_bwd_kernel1, dim3(grid_for(n, 256, 256 * 16)), dim3(256), 0, s, dy, u, us, scale, dx, dxs, n, C);
  return check_launch("vp_affine_relu_bwd_f32");
}

size_t vp_bce_masked_rows_bwd_workspace_bytes(int rows, int n) { return vp_bce_rows_workspace_bytes(rows, n); }

int vp_bce_masked_rows_bwd_f32(const float* p, const float* t, const float* mask, int rows, int n, float* out, float* dlogit, void* ws,
                               size_t ws_bytes, vp_stream stream) {
  VP_REQUIRE(p && t && out && dlogit && ws && rows > 0 && n > 0, "vp_bce_masked_rows_bwd_f32: bad arguments");
  VP_REQUIRE(score_chunks(n) <= 65535, "vp_bce_masked_rows_bwd_f32: rows longer than 65535 x %d elements", SCORE_CHUNK);
  if (ws_bytes < vp_bce_masked_rows_bwd_workspace_bytes(rows, n))
    return fail(VP_ERR_WORKSPACE, "vp_bce_masked_rows_bwd_f32: workspace too small");
  return bce_rows_launch<true>(p, t, mask, rows, n, out, dlogit, ws, (hipStream_t)stream, "vp_bce_masked_rows_bwd_f32");
}

int vp_latent_adam_f32(float* z, const float* g, float* m, float* v, int* step_count, int rows, int Z, float lr, float beta1,
                       float beta2, float eps, float prior_weight, float* prior, vp_stream stream) {
  VP_REQUIRE(z && rows > 0 && Z > 0, "vp_latent_adam_f32: bad arguments");
  const bool update = g && m && v && step_count, prior_only = !g && !m && !v && !step_count && prior;
  VP_REQUIRE(update || prior_only, "vp_latent_adam_f32: g, m, v and the step counter are given together (the update) or not at all (prior alone)");
  VP_REQUIRE(!update || (beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f), "vp_latent_adam_f32: betas must lie in [0, 1)");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(latent_adam_kernel, dim3(rows), dim3(64), 0, s, z, g, m, v, (const int*)step_count, Z, lr, beta1, beta2, eps,
                     prior_weight, prior);
  int rc = check_launch("vp_latent_adam_f32");
  if (rc || !update) return rc;
  hipLaunchKernelGGL(latent_step_advance_kernel, dim3(1), dim3(1), 0, s, step_count);
  return check_launch("vp_latent_adam_f32(advance)");
}

}  // extern "C"
