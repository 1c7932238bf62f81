// The Style-GAN discriminator's output stage (models/network_Style_GAN.py:214-229), forward and backward, fp32:
//   adv[b] = sigmoid(conv3x3_s2_p1(h_adv; w_adv (1, C, 3, 3)) + b_adv),   aux[b, :] = softmax(conv3x3_s2_p1(h_aux; w_aux (K, C, 3, 3)) + b_aux)
// on 2 x 2 inputs.  The single output pixel sits over input rows / columns -1..1, so of the nine taps only (i + 1, j + 1) with
// i, j in {0, 1} meet data and the other five read padding: the stage is 1 + K dot products of length 4C per image,
//   logit[b, k] = bias[k] + sum_{p = 2i + j, c} h[b, p, c] * w[k, c, i + 1, j + 1],
// with h the NHWC storage [B][4][C] and w as nn.Conv2d stores it (tap (i + 1, j + 1) of channel c at (k * C + c) * 9 + 3i + j + 4).
//
//   forward   one workgroup of four waves per image.  A lane owns the elements e, e + 256, ... of the image's 4C (float4 when
//             C % 4 == 0 and the pointers are 16-byte aligned, else float); per output: a serial sum per lane, an xor butterfly per
//             wave, the four wave partials added in order by one thread; then sigmoid and a max-subtracted softmax.
//   backward  one launch of two kinds of workgroup.  The first B, one per image, turn (d_adv, d_aux) into the logit gradients
//             da = d_adv adv (1 - adv), du = aux (d_aux - sum_k aux_k d_aux_k) and write dh = sum_k d[k] w[k] over the live taps.  The
//             rest each own one output k and 256 elements of its dw: every thread recomputes the logit gradient of an image in turn
//             (tiles of 256 images through LDS), sums d[b, k] h[b, e] over b serially in registers, stores its live tap and the
//             dead taps next to it as 0.0f; the first of them sums db[k] from the same tiles.
// Every sum has a fixed order and there is no atomic: two runs give the same bits.  No workspace.
#include "common.h"
#include <cstdint>

namespace vp {
namespace {

constexpr int kHeadMaxC = 1024;
constexpr int kHeadMaxK = 64;

__device__ __forceinline__ float head_sigmoid(float z) {
  const float e = expf(-fabsf(z));
  return z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// element e of an image's [4][C] block, in units of T: its pixel, first channel, and offset of its live tap inside w[k]
template <typename T>
struct HeadElem {
  static constexpr int W = sizeof(T) / 4;
  int p, c, woff;
  __device__ __forceinline__ HeadElem(int e, int C) {
    const int f = e * W;
    p = f / C;
    c = f - p * C;
    woff = c * 9 + 3 * (p >> 1) + (p & 1) + 4;
  }
};

// the W live-tap weights that meet element e (channels c .. c + W - 1 are 9 floats apart)
__device__ __forceinline__ float head_w(const float* __restrict__ w, int woff, float) { return w[woff]; }
__device__ __forceinline__ float4 head_w(const float* __restrict__ w, int woff, float4) {
  return make_float4(w[woff], w[woff + 9], w[woff + 18], w[woff + 27]);
}
__device__ __forceinline__ float head_dot(float a, float b) { return a * b; }
__device__ __forceinline__ float head_dot(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
__device__ __forceinline__ void head_axpy(float& a, float s, float v) { a += s * v; }
__device__ __forceinline__ void head_axpy(float4& a, float s, float4 v) {
  a.x += s * v.x;
  a.y += s * v.y;
  a.z += s * v.z;
  a.w += s * v.w;
}
__device__ __forceinline__ void head_zero(float& a) { a = 0.f; }
__device__ __forceinline__ void head_zero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float head_get(float a, int) { return a; }
__device__ __forceinline__ float head_get(float4 a, int q) { return q == 0 ? a.x : q == 1 ? a.y : q == 2 ? a.z : a.w; }

// ---- forward: one workgroup per image --------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) twin_head_fwd_kernel(const float* __restrict__ h_adv, const float* __restrict__ h_aux,
                                                            const float* __restrict__ w_adv, const float* __restrict__ b_adv,
                                                            const float* __restrict__ w_aux, const float* __restrict__ b_aux,
                                                            float* __restrict__ adv, float* __restrict__ aux, int C, int K) {
  constexpr int W = sizeof(T) / 4;
  __shared__ float part[kHeadMaxK + 1][4], logit[kHeadMaxK + 1];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nel = 4 * C / W;
  const T* ha = reinterpret_cast<const T*>(h_adv + (size_t)b * 4 * C);
  const T* hu = reinterpret_cast<const T*>(h_aux + (size_t)b * 4 * C);
  for (int o = 0; o <= K; ++o) {      // output 0 is the adversarial logit, 1 + k the class logit k
    const T* h = o == 0 ? ha : hu;
    const float* w = o == 0 ? w_adv : w_aux + (size_t)(o - 1) * C * 9;
    float a = 0.f;
    for (int e = tid; e < nel; e += 256) {
      const HeadElem<T> el(e, C);
      a += head_dot(h[e], head_w(w, el.woff, T()));
    }
    a = wave_sum(a);
    if (lane == 0) part[o][wave] = a;
  }
  __syncthreads();
  if (tid <= K) logit[tid] = (tid == 0 ? b_adv[0] : b_aux[tid - 1]) + (((part[tid][0] + part[tid][1]) + part[tid][2]) + part[tid][3]);
  __syncthreads();
  if (tid == 0) adv[b] = head_sigmoid(logit[0]);
  if (tid >= 1 && tid <= K) {         // every class thread walks the K logits in the same order: the same maximum and sum in all
    float m = logit[1];
    for (int k = 2; k <= K; ++k) m = fmaxf(m, logit[k]);
    float s = 0.f;
    for (int k = 1; k <= K; ++k) s += expf(logit[k] - m);
    aux[(size_t)b * K + tid - 1] = expf(logit[tid] - m) / s;
  }
}

// gradient of the logit of output o (0: adversarial, 1 + k: class k) of image b; a null d_adv / d_aux is a zero gradient
__device__ __forceinline__ float head_dlogit(const float* __restrict__ adv, const float* __restrict__ aux,
                                             const float* __restrict__ d_adv, const float* __restrict__ d_aux, size_t b, int o, int K) {
  if (o == 0) {
    const float y = adv[b], g = d_adv ? d_adv[b] : 0.f;
    return g * y * (1.f - y);
  }
  if (!d_aux) return 0.f;
  const float* y = aux + b * K;
  const float* g = d_aux + b * K;
  float s = 0.f;
  for (int k = 0; k < K; ++k) s += y[k] * g[k];
  return y[o - 1] * (g[o - 1] - s);
}

// ---- backward: workgroups [0, B) write dh of one image each, the others one (output, 256-element) slice of dw [and db] each ----------
template <typename T>
__global__ void __launch_bounds__(256) twin_head_bwd_kernel(const float* __restrict__ h_adv, const float* __restrict__ h_aux,
                                                            const float* __restrict__ w_adv, const float* __restrict__ w_aux,
                                                            const float* __restrict__ adv, const float* __restrict__ aux,
                                                            const float* __restrict__ d_adv, const float* __restrict__ d_aux,
                                                            float* __restrict__ dh_adv, float* __restrict__ dh_aux,
                                                            float* __restrict__ dw_adv, float* __restrict__ db_adv,
                                                            float* __restrict__ dw_aux, float* __restrict__ db_aux, int B, int C, int K,
                                                            int nslice) {
  constexpr int W = sizeof(T) / 4;
  __shared__ float sd[256];
  const int tid = threadIdx.x, nel = 4 * C / W;
  if ((int)blockIdx.x < B) {
    const size_t b = blockIdx.x;
    if (tid <= K) sd[tid] = head_dlogit(adv, aux, d_adv, d_aux, b, tid, K);
    __syncthreads();
    T* oa = reinterpret_cast<T*>(dh_adv + b * 4 * C);
    T* ou = reinterpret_cast<T*>(dh_aux + b * 4 * C);
    for (int e = tid; e < nel; e += 256) {
      const HeadElem<T> el(e, C);
      T a, u;
      head_zero(a);
      head_zero(u);
      head_axpy(a, sd[0], head_w(w_adv, el.woff, T()));
      for (int k = 0; k < K; ++k) head_axpy(u, sd[1 + k], head_w(w_aux + (size_t)k * C * 9, el.woff, T()));
      oa[e] = a;
      ou[e] = u;
    }
    return;
  }
  const int j = blockIdx.x - B, o = j / nslice, slice = j - o * nslice, e = slice * 256 + tid;
  const float* h = o == 0 ? h_adv : h_aux;
  float* dw = o == 0 ? dw_adv : dw_aux + (size_t)(o - 1) * C * 9;
  T acc;
  head_zero(acc);
  float bsum = 0.f;
  for (int b0 = 0; b0 < B; b0 += 256) {
    const int nb = min(256, B - b0);
    __syncthreads();
    if (tid < nb) sd[tid] = head_dlogit(adv, aux, d_adv, d_aux, (size_t)(b0 + tid), o, K);
    __syncthreads();
    if (e < nel) {
      const T* hp = reinterpret_cast<const T*>(h + (size_t)b0 * 4 * C) + e;
#pragma unroll 4
      for (int i = 0; i < nb; ++i) head_axpy(acc, sd[i], hp[(size_t)i * nel]);
    }
    if (slice == 0 && tid == 0)
      for (int i = 0; i < nb; ++i) bsum += sd[i];
  }
  if (slice == 0 && tid == 0) (o == 0 ? db_adv : db_aux + (o - 1))[0] = bsum;
  if (e >= nel) return;
  const HeadElem<T> el(e, C);
#pragma unroll
  for (int q = 0; q < W; ++q) {
    float* row = dw + (size_t)(el.c + q) * 9;      // the nine taps of channel c + q; pixel p owns the live tap 3i + j + 4 ...
    row[3 * (el.p >> 1) + (el.p & 1) + 4] = head_get(acc, q);
    if (el.p == 0) row[0] = row[1] = row[2] = 0.f;   // ... and between them the four pixels zero row 0 and column 0
    if (el.p == 1) row[3] = 0.f;
    if (el.p == 2) row[6] = 0.f;
  }
}

inline bool head_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int twin_head_check_dims(const char* who, int B, int C, int K) {
  VP_REQUIRE(B > 0, "%s: B must be positive", who);
  VP_REQUIRE(C >= 1 && C <= kHeadMaxC, "%s: C = %d is not supported (1 <= C <= %d)", who, C, kHeadMaxC);
  VP_REQUIRE(K >= 1 && K <= kHeadMaxK, "%s: K = %d classes are not supported (1 <= K <= %d)", who, K, kHeadMaxK);
  return VP_OK;
}

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" int vp_twin_head_fwd_f32(const float* h_adv, const float* h_aux, const float* w_adv, const float* b_adv, const float* w_aux,
                                    const float* b_aux, float* adv, float* aux, int B, int C, int K, vp_stream stream) {
  if (int rc = twin_head_check_dims("vp_twin_head_fwd_f32", B, C, K)) return rc;
  VP_REQUIRE(h_adv && h_aux && w_adv && b_adv && w_aux && b_aux && adv && aux, "vp_twin_head_fwd_f32: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(B), blk(256);
  if (C % 4 == 0 && head_aligned16(h_adv) && head_aligned16(h_aux))
    hipLaunchKernelGGL(twin_head_fwd_kernel<float4>, grid, blk, 0, s, h_adv, h_aux, w_adv, b_adv, w_aux, b_aux, adv, aux, C, K);
  else
    hipLaunchKernelGGL(twin_head_fwd_kernel<float>, grid, blk, 0, s, h_adv, h_aux, w_adv, b_adv, w_aux, b_aux, adv, aux, C, K);
  return check_launch("vp_twin_head_fwd_f32");
}

extern "C" int vp_twin_head_bwd_f32(const float* h_adv, const float* h_aux, const float* w_adv, const float* w_aux, const float* adv,
                                    const float* aux, const float* d_adv, const float* d_aux, float* dh_adv, float* dh_aux,
                                    float* dw_adv, float* db_adv, float* dw_aux, float* db_aux, int B, int C, int K, vp_stream stream) {
  if (int rc = twin_head_check_dims("vp_twin_head_bwd_f32", B, C, K)) return rc;
  VP_REQUIRE(h_adv && h_aux && w_adv && w_aux && adv && aux && dh_adv && dh_aux && dw_adv && db_adv && dw_aux && db_aux,
             "vp_twin_head_bwd_f32: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = C % 4 == 0 && head_aligned16(h_adv) && head_aligned16(h_aux) && head_aligned16(dh_adv) && head_aligned16(dh_aux);
  const int nel = vec ? C : 4 * C, nslice = (nel + 255) / 256;
  const long long blocks = (long long)B + (long long)(1 + K) * nslice;
  VP_REQUIRE(blocks <= 0x7fffffffLL, "vp_twin_head_bwd_f32: B = %d exceeds the grid", B);
  const dim3 grid((unsigned)blocks), blk(256);
  if (vec)
    hipLaunchKernelGGL(twin_head_bwd_kernel<float4>, grid, blk, 0, s, h_adv, h_aux, w_adv, w_aux, adv, aux, d_adv, d_aux, dh_adv, dh_aux,
                       dw_adv, db_adv, dw_aux, db_aux, B, C, K, nslice);
  else
    hipLaunchKernelGGL(twin_head_bwd_kernel<float>, grid, blk, 0, s, h_adv, h_aux, w_adv, w_aux, adv, aux, d_adv, d_aux, dh_adv, dh_aux,
                       dw_adv, db_adv, dw_aux, db_aux, B, C, K, nslice);
  return check_launch("vp_twin_head_bwd_f32");
}
