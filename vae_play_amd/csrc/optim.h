// torch.optim.Adam's single-tensor update (no amsgrad, no weight decay), stated once with every rounding written out:
//   g' = grad_scale g;  m.lerp_(g', 1-b1);  v = v b2 + (1-b2) g' g';  denom = sqrt(v)/sqrt(bc2) + eps;  p -= (lr/bc1) m/denom
// Used by adam_kernel and adam_outer_kernel (optim.hip) and latent_adam_kernel (project.hip).  DESIGN.md section 25.
#pragma once
#include <cmath>
#include "common.h"

namespace vp {

// the constants of step `step` (1-based), the bias corrections in double; on the host for vp_adam_f32 / vp_adam_outer_f32, on the
// device for latent_adam_kernel, which reads its step count from device memory
struct AdamStep { float one_minus_b1, b2, one_minus_b2, eps, step_size, bc2_sqrt; };
__host__ __device__ inline AdamStep adam_step_constants(float lr, float beta1, float beta2, float eps, int step) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  return {1.f - beta1, beta2, 1.f - beta2, eps, (float)((double)lr / bc1), (float)sqrt(bc2)};
}

// How v's two products are fused.  The update used to be an expression left to the compiler, which fused it differently from path
// to path; each path now names the form it was observed to take, so the bits no longer depend on the compiler.  With
// gg = ((1-b2) g') g' rounded:
enum AdamVForm {
  ADAM_V_FMA_SQUARE,      // v = fma(g', (1-b2) g', b2 v)   b2 v rounded, the square fused
  ADAM_V_FMA_DECAY,       // v = fma(b2, v, gg)             the square rounded, the decay fused
  ADAM_V_TWO_PRODUCTS,    // v = b2 v + gg                  both products rounded
};

// adam_outer_kernel<8>, row u of a group of four rows (row % 4) and column c of the thread's quad (column % 4)
__host__ __device__ constexpr AdamVForm adam_outer_v_form(int u, int c) {
  return u < 3 && c < 2 ? ADAM_V_FMA_SQUARE : ADAM_V_TWO_PRODUCTS;
}

// m and p take one form on every path: m = fma(1-b1, fma(grad_scale, g, -m), m), p = fma(-lr/bc1, m/denom, p).
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, AdamVForm form, float grad_scale, const AdamStep& k) {
#pragma clang fp contract(off)
  const float gr = g * grad_scale;
  m = fmaf(k.one_minus_b1, fmaf(grad_scale, g, -m), m);
  const float t = k.one_minus_b2 * gr;
  if (form == ADAM_V_FMA_SQUARE) v = fmaf(gr, t, k.b2 * v);
  else if (form == ADAM_V_FMA_DECAY) v = fmaf(k.b2, v, t * gr);
  else v = v * k.b2 + t * gr;
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
  p = fmaf(-k.step_size, m / denom, p);
}

}  // namespace vp
