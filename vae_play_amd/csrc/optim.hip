// The fused flat-arena optimiser steps: Adam, Adam on a gradient given as a sum of outer products, RMSprop.  HBM-bound.
#include "optim.h"
#include "problems.h"

namespace vp {

template <AdamVForm FORM>
__device__ __forceinline__ void adam_update4(vp_f32x4& pv, const vp_f32x4& gv, vp_f32x4& mv, vp_f32x4& vv, float grad_scale,
                                             const AdamStep& k) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float p = pv[j], m = mv[j], v = vv[j];
    adam_update(p, gv[j], m, v, FORM, grad_scale, k);
    pv[j] = p; mv[j] = m; vv[j] = v;
  }
}

// The three paths of the walk take three forms of v (optim.h): the form the compiler gave each when the update was one expression.
__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, size_t n, float one_minus_b1, float b2,
                                                   float one_minus_b2, float eps, float step_size, float bc2_sqrt,
                                                   float grad_scale) {
  const AdamStep k = {one_minus_b1, b2, one_minus_b2, eps, step_size, bc2_sqrt};
  const size_t n4 = n / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  // two independent 16-B quads per thread and iteration: 8 loads in flight before the first use; the moments
  // are streamed with non-temporal accesses (touched once per step), p and g stay cacheable for their consumers
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    const size_t a = i * 4, b = (i + stride) * 4;
    vp_f32x4 pa = *reinterpret_cast<vp_f32x4*>(p + a), pb = *reinterpret_cast<vp_f32x4*>(p + b);
    vp_f32x4 ga = *reinterpret_cast<const vp_f32x4*>(g + a), gb = *reinterpret_cast<const vp_f32x4*>(g + b);
    vp_f32x4 ma = __builtin_nontemporal_load(reinterpret_cast<vp_f32x4*>(m + a));
    vp_f32x4 mb = __builtin_nontemporal_load(reinterpret_cast<vp_f32x4*>(m + b));
    vp_f32x4 va = __builtin_nontemporal_load(reinterpret_cast<vp_f32x4*>(v + a));
    vp_f32x4 vb = __builtin_nontemporal_load(reinterpret_cast<vp_f32x4*>(v + b));
    adam_update4<ADAM_V_FMA_SQUARE>(pa, ga, ma, va, grad_scale, k);
    adam_update4<ADAM_V_FMA_SQUARE>(pb, gb, mb, vb, grad_scale, k);
    *reinterpret_cast<vp_f32x4*>(p + a) = pa;
    *reinterpret_cast<vp_f32x4*>(p + b) = pb;
    __builtin_nontemporal_store(ma, reinterpret_cast<vp_f32x4*>(m + a));
    __builtin_nontemporal_store(mb, reinterpret_cast<vp_f32x4*>(m + b));
    __builtin_nontemporal_store(va, reinterpret_cast<vp_f32x4*>(v + a));
    __builtin_nontemporal_store(vb, reinterpret_cast<vp_f32x4*>(v + b));
  }
  if (i < n4) {
    const size_t a = i * 4;
    vp_f32x4 pa = *reinterpret_cast<vp_f32x4*>(p + a);
    vp_f32x4 ga = *reinterpret_cast<const vp_f32x4*>(g + a);
    vp_f32x4 ma = *reinterpret_cast<vp_f32x4*>(m + a), va = *reinterpret_cast<vp_f32x4*>(v + a);
    adam_update4<ADAM_V_FMA_DECAY>(pa, ga, ma, va, grad_scale, k);
    *reinterpret_cast<vp_f32x4*>(p + a) = pa;
    *reinterpret_cast<vp_f32x4*>(m + a) = ma;
    *reinterpret_cast<vp_f32x4*>(v + a) = va;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t i = n4 * 4 + threadIdx.x;
    float pp = p[i], mm = m[i], vv = v[i];
    adam_update(pp, g[i], mm, vv, ADAM_V_TWO_PRODUCTS, grad_scale, k);
    m[i] = mm; v[i] = vv;
    p[i] = pp;
  }
}

// Adam update of a weight matrix p[R][Cn] whose gradient is a sum of K outer products, g = grad_scale * A^T B with A [K][R] and
// B [K][Cn] (a Linear layer's weight gradient: A = the output gradients, B = the inputs of the K samples).  The gradient is
// contracted in registers and consumed at once: for the encoder's first dense layer (1024 x 32768, 63 % of the model's parameters,
// K = 32 images) that saves writing and re-reading a 134-MB gradient matrix per step.  One workgroup = 8 rows x 1024 columns,
// one thread = 8 rows x 4 columns (32 accumulators); per k it loads one 16-B quad of B and 8 wave-uniform values of A.
// (16 rows per thread measured 150 us against 142 us on the 1024 x 32768 layer.)
template <int AO_TI>
__global__ void __launch_bounds__(256) adam_outer_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                         const float* __restrict__ A, const float* __restrict__ Bm, int K, int R, int Cn,
                                                         float one_minus_b1, float b2, float one_minus_b2, float eps, float step_size,
                                                         float bc2_sqrt, float grad_scale) {
  const AdamStep ks = {one_minus_b1, b2, one_minus_b2, eps, step_size, bc2_sqrt};
  const int j = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int i0 = blockIdx.y * AO_TI;
  if (j >= Cn) return;
  float acc[AO_TI][4];
#pragma unroll
  for (int i = 0; i < AO_TI; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = 0.f;
  const bool full = i0 + AO_TI <= R;
  auto kstep = [&](int k) {
    const vp_f32x4 b4 = *reinterpret_cast<const vp_f32x4*>(Bm + (size_t)k * Cn + j);
    const float* ak = A + (size_t)k * R + i0;
    float a[AO_TI];
    if (full) {
#pragma unroll
      for (int q = 0; q < AO_TI / 4; ++q) {
        const vp_f32x4 t = *reinterpret_cast<const vp_f32x4*>(ak + 4 * q);
        a[4 * q] = t[0]; a[4 * q + 1] = t[1]; a[4 * q + 2] = t[2]; a[4 * q + 3] = t[3];
      }
    } else {
#pragma unroll
      for (int i = 0; i < AO_TI; ++i) a[i] = i0 + i < R ? ak[i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < AO_TI; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(a[i], b4[c], acc[i][c]);
  };
  int k = 0;
  for (; k + 4 <= K; k += 4) {      // four k per trip: their loads are issued together
    kstep(k); kstep(k + 1); kstep(k + 2); kstep(k + 3);
  }
  for (; k < K; ++k) kstep(k);
  // rows in groups of four: 12 independent 16-B loads in flight before the first use (every row index is a compile-time
  // constant: a runtime index would send the accumulators to scratch)
#pragma unroll
  for (int i4 = 0; i4 < AO_TI; i4 += 4) {
    vp_f32x4 pv[4], mv[4], vv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = i0 + i4 + u;
      const size_t o = (size_t)(r < R ? r : R - 1) * Cn + j;         // (rows past the end: clamped load, no store)
      pv[u] = *reinterpret_cast<vp_f32x4*>(p + o);
      mv[u] = __builtin_nontemporal_load(reinterpret_cast<vp_f32x4*>(m + o));
      vv[u] = __builtin_nontemporal_load(reinterpret_cast<vp_f32x4*>(v + o));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = i0 + i4 + u;
      if (r >= R) continue;
      const size_t o = (size_t)r * Cn + j;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float pp = pv[u][c], mm = mv[u][c], v1 = vv[u][c];
        adam_update(pp, acc[i4 + u][c], mm, v1, adam_outer_v_form(u, c), grad_scale, ks);
        pv[u][c] = pp; mv[u][c] = mm; vv[u][c] = v1;
      }
      *reinterpret_cast<vp_f32x4*>(p + o) = pv[u];
      __builtin_nontemporal_store(mv[u], reinterpret_cast<vp_f32x4*>(m + o));
      __builtin_nontemporal_store(vv[u], reinterpret_cast<vp_f32x4*>(v + o));
    }
  }
}

// torch.optim.RMSprop: sq = alpha*sq + (1-alpha)*g*g; p -= lr * g / (sqrt(sq) + eps)
__global__ void __launch_bounds__(256) rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq,
                                                      size_t n, float lr, float alpha, float one_minus_alpha, float eps,
                                                      float grad_scale) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float gr = g[i] * grad_scale;
    const float s = sq[i] * alpha + one_minus_alpha * gr * gr;
    sq[i] = s;
    p[i] = p[i] - lr * (gr / (sqrtf(s) + eps));
  }
}

}  // namespace vp

using namespace vp;

extern "C" {

int vp_adam_f32(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps, int step,
                float grad_scale, vp_stream stream) {
  VP_REQUIRE(p && g && m && v && n > 0 && step >= 1, "vp_adam_f32: bad arguments");
  VP_REQUIRE(aligned16(p, g, m, v), "vp_adam_f32: arena must be 16-byte aligned");
  const AdamStep k = adam_step_constants(lr, beta1, beta2, eps, step);
  return launch_flat("vp_adam_f32", adam_kernel, n / 4 + 1, 256 * 64, (hipStream_t)stream, p, g, m, v, n, k.one_minus_b1, k.b2,
                     k.one_minus_b2, k.eps, k.step_size, k.bc2_sqrt, grad_scale);
}

int vp_adam_outer_f32(float* p, float* m, float* v, const float* A, const float* Bm, int K, int R, int Cn, float lr, float beta1,
                      float beta2, float eps, int step, float grad_scale, vp_stream stream) {
  VP_REQUIRE(p && m && v && A && Bm && K > 0 && R > 0 && Cn > 0 && step >= 1, "vp_adam_outer_f32: bad arguments");
  VP_REQUIRE(Cn % 4 == 0 && R % 4 == 0, "vp_adam_outer_f32: R and Cn must be multiples of 4");
  const AdamStep k = adam_step_constants(lr, beta1, beta2, eps, step);
  const dim3 grid((unsigned)((Cn / 4 + 255) / 256), (unsigned)((R + 7) / 8));
  VP_REQUIRE(grid.y <= 65535, "vp_adam_outer_f32: too many rows");
  hipLaunchKernelGGL(adam_outer_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, p, m, v, A, Bm, K, R, Cn, k.one_minus_b1, k.b2,
                     k.one_minus_b2, k.eps, k.step_size, k.bc2_sqrt, grad_scale);
  return check_launch("vp_adam_outer_f32");
}

int vp_rmsprop_f32(float* p, const float* g, float* sq, size_t n, float lr, float alpha, float eps, float grad_scale,
                   vp_stream stream) {
  VP_REQUIRE(p && g && sq && n > 0, "vp_rmsprop_f32: bad arguments");
  return launch_flat("vp_rmsprop_f32", rmsprop_kernel, n, 256 * 16, (hipStream_t)stream, p, g, sq, n, lr, alpha, 1.f - alpha, eps,
                     grad_scale);
}

}  // extern "C"
