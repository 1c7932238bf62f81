// Kernels of fused VAE-GAN inference (vae_play_amd/infer_gan.py): the discriminator's tap and head in eval mode, and the fold of a chain
// of bias-ed Linear layers without activations (DirectDecoder, models/networks.py:118-148) into one affine map.
//
//   vp_disc_tap_eval_f32   the tap block (conv[recon_level], models/networks.py:178-183) after its convolution: reads the fp32 NHWC
//                          output c [n][64][C] once and writes, in the reference's NCHW flatten order, the eval-mode BatchNorm + ReLU
//                          relu(fma(c, s, t)) (what fc.0 reads), c itself (the "REC" features) and, per image pair (i, i + P), the
//                          feature distance 1/2 sum (c[i] - c[i + P])^2 ("mse", :273).  It stands in for a normalise pass, a
//                          transpose, a second transpose for the features and the row sum.
//   vp_disc_head_eval_f32  fc.1 (eval BatchNorm + ReLU), fc.3, the sigmoid and -log(p + 1e-3), -log(1 - p + 1e-3) (:198, :274-276)
//   vp_lin_fold_f32        W_new = W_out W, b_new = W_out b + b_out for at most 8 output rows
//
// Every sum has one fixed order that depends on the row (or row pair) alone: not on n, not on the grid.  No atomics.
#include "common.h"

namespace vp {

// One workgroup per image pair (i, i + P) for i < P, one per image for the images from 2P on.  The 64 x C image goes through LDS in
// tiles of 64 pixels x 32 channels: 128-B rows in, 32 x 64 consecutive floats out (a tile IS a contiguous piece of the NCHW-flat row).
// The workgroup is TAP_G groups of 256 threads; group g takes tiles g, g + TAP_G, ... and requests its next tile before it reads the
// current one out of LDS (a pair's distance needs ONE workgroup per pair -- no atomics, no workspace -- so with few pairs the
// kernel is latency-bound: the groups and the prefetch are what keeps loads in flight).
// A thread's elements, the order it adds them in and the tree over the waves are the same for every call: the distance is
// bit-reproducible and the same whether the pair sits in a batch of 2 or of 64.
constexpr int TAP_PITCH = 65, TAP_G = 2;
__global__ void __launch_bounds__(256 * TAP_G) disc_tap_eval_kernel(const float* __restrict__ c, const float* __restrict__ scale,
                                                                    const float* __restrict__ shift, int C, float* __restrict__ act_flat,
                                                                    float* __restrict__ feat_flat, int P, float* __restrict__ dist) {
  __shared__ float tile[TAP_G][2][32 * TAP_PITCH];
  __shared__ double sh[4 * TAP_G];
  const int t = threadIdx.x & 255, grp = threadIdx.x >> 8;
  const bool pair = (int)blockIdx.x < P;
  const int img0 = pair ? (int)blockIdx.x : (int)blockIdx.x + P;
  const int nimg = pair ? 2 : 1;
  const size_t row = (size_t)64 * C;
  const int ntiles = C / 32;
  vp_f32x4 v[2][2];
  auto load = [&](int ct) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int f = t + 256 * k, px = f >> 3, ch = (f & 7) * 4;
#pragma unroll
      for (int g = 0; g < 2; ++g)
        if (g < nimg) v[g][k] = *reinterpret_cast<const vp_f32x4*>(c + (size_t)(img0 + g * P) * row + (size_t)px * C + 32 * ct + ch);
    }
  };
  float acc = 0.f;
  int ct = grp;
  if (ct < ntiles) load(ct);
  for (int it = 0; it < (ntiles + TAP_G - 1) / TAP_G; ++it, ct += TAP_G) {      // (the same trip count for every group: the barriers)
    const bool live = ct < ntiles;
    __syncthreads();                       // the previous tile's reads are done
    if (live) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int f = t + 256 * k, px = f >> 3, ch = (f & 7) * 4;
#pragma unroll
        for (int g = 0; g < 2; ++g)
          if (g < nimg) {
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[grp][g][(ch + j) * TAP_PITCH + px] = v[g][k][j];
          }
      }
    }
    __syncthreads();
    if (ct + TAP_G < ntiles) load(ct + TAP_G);
    if (!live) continue;
    const int c0 = 32 * ct;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int o4 = t + 256 * k, ch = o4 >> 4, p4 = (o4 & 15) * 4;
      const float s = act_flat ? scale[c0 + ch] : 0.f, sf = act_flat ? shift[c0 + ch] : 0.f;
      vp_f32x4 x[2];
#pragma unroll
      for (int g = 0; g < 2; ++g)
        if (g < nimg) {
#pragma unroll
          for (int j = 0; j < 4; ++j) x[g][j] = tile[grp][g][ch * TAP_PITCH + p4 + j];
          const size_t o = (size_t)(img0 + g * P) * row + (size_t)(c0 + ch) * 64 + p4;
          if (feat_flat) *reinterpret_cast<vp_f32x4*>(feat_flat + o) = x[g];
          if (act_flat) {
            vp_f32x4 a;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float y = __builtin_fmaf(x[g][j], s, sf);      // ONE rounding, as the convolutions' affine epilogue
              a[j] = y > 0.f ? y : 0.f;
            }
            *reinterpret_cast<vp_f32x4*>(act_flat + o) = a;
          }
        }
      if (pair) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d = x[0][j] - x[1][j];
          acc += 0.5f * d * d;
        }
      }
    }
  }
  if (pair && dist) {                      // (uniform over the workgroup)
    const double w = wave_sum((double)acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
      double tot = 0.0;                    // per group block_sum4's tree, the groups in order
#pragma unroll
      for (int g = 0; g < TAP_G; ++g) tot += (sh[4 * g] + sh[4 * g + 1]) + (sh[4 * g + 2] + sh[4 * g + 3]);
      dist[blockIdx.x] = (float)tot;
    }
  }
}

// One wavefront per row: lane l takes columns l, l + 64, ...; the products -- exact in fp64 -- are added in fp64 in that order, then
// the wave tree.  The logit is therefore the correctly rounded sum up to fp64's error, whatever cancels in it.
__global__ void __launch_bounds__(64) disc_head_eval_kernel(const float* __restrict__ h, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, const float* __restrict__ w,
                                                            const float* __restrict__ bias, int H, float* __restrict__ logit,
                                                            float* __restrict__ p_out, float* __restrict__ nl_real,
                                                            float* __restrict__ nl_fake) {
  const int r = blockIdx.x;
  const float* hr = h + (size_t)r * H;
  double acc = 0.0;
  for (int j = threadIdx.x; j < H; j += 64) {
    const float y = __builtin_fmaf(hr[j], scale[j], shift[j]);
    acc += (double)(y > 0.f ? y : 0.f) * (double)w[j];
  }
  acc = wave_sum(acc);
  if (threadIdx.x == 0) {
    const float x = (float)(acc + (double)bias[0]);
    float p, q;
    sigmoid_pair(x, expf(-fabsf(x)), p, q);      // q = 1 - p without the cancellation, as the GAN head of the training step
    if (logit) logit[r] = x;
    if (p_out) p_out[r] = p;
    if (nl_real) nl_real[r] = neg_log_floor(p, q);
    if (nl_fake) nl_fake[r] = neg_log_floor(q, p);
  }
}

// Thread k < K owns column k of W_new, thread K the bias: acc[m] = fma(W_out[m][n], W[n][k], acc[m]) for n = 0 .. N - 1 in that order.
// The reads of W[n][.] are coalesced over the threads; W_out[m][n] is the same address for all of them.
constexpr int FOLD_M = 8;
__global__ void __launch_bounds__(256) lin_fold_kernel(const float* __restrict__ w_out, const float* __restrict__ b_out,
                                                       const float* __restrict__ w, const float* __restrict__ b, int M, int N, int K,
                                                       float* __restrict__ w_new, float* __restrict__ b_new) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k > K) return;
  const bool is_bias = k == K;
  float acc[FOLD_M];
#pragma unroll
  for (int m = 0; m < FOLD_M; ++m) acc[m] = (is_bias && m < M) ? b_out[m] : 0.f;
  for (int n = 0; n < N; ++n) {
    const float x = is_bias ? b[n] : w[(size_t)n * K + k];
#pragma unroll
    for (int m = 0; m < FOLD_M; ++m)
      if (m < M) acc[m] = __builtin_fmaf(w_out[(size_t)m * N + n], x, acc[m]);
  }
#pragma unroll
  for (int m = 0; m < FOLD_M; ++m)
    if (m < M) {
      if (is_bias) b_new[m] = acc[m];
      else w_new[(size_t)m * K + k] = acc[m];
    }
}

}  // namespace vp

using namespace vp;

extern "C" {

int vp_disc_tap_eval_f32(const float* c, const float* scale, const float* shift, int n, int C, float* act_flat, float* feat_flat,
                         int pair_rows, float* dist, vp_stream stream) {
  VP_REQUIRE(c && n > 0 && C > 0 && C % 32 == 0, "vp_disc_tap_eval_f32: needs n > 0 images of 8 x 8 x C, C a multiple of 32");
  VP_REQUIRE(act_flat || feat_flat || (dist && pair_rows > 0), "vp_disc_tap_eval_f32: nothing to write");
  VP_REQUIRE(!act_flat || (scale && shift), "vp_disc_tap_eval_f32: act_flat needs scale and shift");
  VP_REQUIRE(pair_rows >= 0 && 2 * (size_t)pair_rows <= (size_t)n, "vp_disc_tap_eval_f32: pair_rows must be at most n / 2");
  VP_REQUIRE(pair_rows == 0 || dist, "vp_disc_tap_eval_f32: pair_rows > 0 needs dist");
  VP_REQUIRE(aligned16(c, act_flat, feat_flat), "vp_disc_tap_eval_f32: c, act_flat and feat_flat must be 16-byte aligned");
  hipLaunchKernelGGL(disc_tap_eval_kernel, dim3(n - pair_rows), dim3(256 * TAP_G), 0, (hipStream_t)stream, c, scale, shift, C, act_flat, feat_flat,
                     pair_rows, dist);
  return check_launch("vp_disc_tap_eval_f32");
}

int vp_disc_head_eval_f32(const float* h, const float* scale, const float* shift, const float* w, const float* bias, int n, int H,
                          float* logit, float* p, float* nl_real, float* nl_fake, vp_stream stream) {
  VP_REQUIRE(h && scale && shift && w && bias && n > 0 && H > 0, "vp_disc_head_eval_f32: bad arguments");
  VP_REQUIRE(logit || p || nl_real || nl_fake, "vp_disc_head_eval_f32: nothing to write");
  hipLaunchKernelGGL(disc_head_eval_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, h, scale, shift, w, bias, H, logit, p, nl_real,
                     nl_fake);
  return check_launch("vp_disc_head_eval_f32");
}

int vp_lin_fold_f32(const float* w_out, const float* b_out, const float* w, const float* b, int M, int N, int K, float* w_new,
                    float* b_new, vp_stream stream) {
  VP_REQUIRE(w_out && b_out && w && b && w_new && b_new && N > 0 && K > 0, "vp_lin_fold_f32: bad arguments");
  VP_REQUIRE(M > 0 && M <= FOLD_M, "vp_lin_fold_f32: 1 to 8 output rows");
  hipLaunchKernelGGL(lin_fold_kernel, dim3(K / 256 + 1), dim3(256), 0, (hipStream_t)stream, w_out, b_out, w, b, M, N, K, w_new, b_new);
  return check_launch("vp_lin_fold_f32");
}

}
