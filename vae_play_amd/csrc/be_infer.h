// Tile bodies of the fused eval-mode mask / edge heads of models/networks_BE.py:39-66 (be_infer.hip), written as
// __host__ __device__ functions over a plain float array that stands for LDS: tests/host_emul/be_infer_emul.cpp compiles this text
// for the host and runs every tile of an image through it.
//
// One workgroup of NT = 256 threads owns a TH x TW tile of a head's map and runs three tile-local stages over it:
//
//   Up block      X (TH+6)x(TW+6)  -conv1 (cin + 2 -> cmid), folded BN, ReLU->  A (TH+4)x(TW+4)
//                                  -conv2 (cmid -> cmid),    folded BN, ReLU->  B (TH+2)x(TW+2)  -2x bilinear->  Y 2TH x 2TW
//   predictor     X (TH+6)x(TW+6)  -conv1 (c -> 2c) + bias->  A  -conv2 (2c -> c) + bias->  B  -conv3 (c -> 1) + bias->  TH x TW logits
//
// The border rules (each region is addressed by its image position, so they are stated once per stage):
//   * X, A and B of the predictor hold 0 at every position outside the image: each convolution pads ITS OWN input with zeros;
//     an intermediate outside the image is never "the previous layer evaluated on padding" (that would be relu(shift) or a bias);
//   * the two coordinate channels of AddCoords (column index, row index, unnormalised; models/blocks.py:106-111) are computed from
//     the tap's image position and exist only inside the image: the convolution's padding ring holds 0 there too;
//   * the resize clamps its source index at the image border, so it only ever reads B at positions inside the image.
//
// A thread is named by ``tid`` in [0, NT).  On the device a phase loop runs once (tid0 = threadIdx.x, TSTEP = NT) and tile_sync() is
// __syncthreads(); on the host the loop walks all NT threads (tid0 = 0, TSTEP = 1) and tile_sync() is nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VP_BE_HD __host__ __device__ __forceinline__
#else
#define VP_BE_HD inline
#endif

namespace vp {
namespace be {

typedef float f4 __attribute__((vector_size(16)));

constexpr int TH = 8, TW = 16, NT = 256;
constexpr int XH = TH + 6, XW = TW + 6;      // input halo tile, origin (h0 - 3, w0 - 3)
constexpr int AH = TH + 4, AW = TW + 4;      // first convolution's outputs, origin (h0 - 2, w0 - 2): 240 pixels, one per thread
constexpr int BH = TH + 2, BW = TW + 2;      // second convolution's outputs, origin (h0 - 1, w0 - 1)
constexpr int CS = 16;                       // input channels of the Up block's first convolution staged per slice
static_assert(AH * AW <= NT && BH * BW <= NT && TH * TW <= NT, "one pixel per thread in every stage");

VP_BE_HD void tile_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}

VP_BE_HD int rnd4(int n) { return (n + 3) & ~3; }
// floats between two pixels of an LDS region with K channels: 16-B aligned pixels (read as f4) when 4 | K, with 4 floats of padding
// so that neighbouring pixels do not start in the same bank group; packed when K = 2 (read as scalars)
VP_BE_HD int pix_stride(int K) { return (K & 3) ? K : K + 4; }
VP_BE_HD bool inside(int h, int w, int H, int W) { return h >= 0 && h < H && w >= 0 && w < W; }

VP_BE_HD bool up_supported(int cin, int cmid) {
  return (cin == 16 && cmid == 4) || (cin == 4 && cmid == 2) || (cin == 32 && cmid == 8) || (cin == 8 && cmid == 4) ||
         (cin == 64 && cmid == 16) || (cin == 16 && cmid == 8);
}
VP_BE_HD bool pred_supported(int c) { return c == 2 || c == 4 || c == 8; }

// ---- packed parameter blocks (global memory, one per head; written by the pack kernels) -------------------------------------------
// Up block: W1 [9][cin + 2][cmid] (tap, input channel -- the two coordinate channels last -- , output channel; the folded BatchNorm
// scale multiplied in), t1 [cmid], W2 [9][cmid][cmid], t2 [cmid]
struct UpParams { int w1, t1, w2, t2, total; };
VP_BE_HD UpParams up_params(int cin, int cmid) {
  UpParams p;
  p.w1 = 0;
  p.t1 = p.w1 + 9 * (cin + 2) * cmid;
  p.w2 = p.t1 + rnd4(cmid);
  p.t2 = p.w2 + rnd4(9 * cmid * cmid);
  p.total = p.t2 + rnd4(cmid);
  return p;
}
// predictor: W1 [9][c][2c], b1 [2c], W2 [9][2c][c], b2 [c], W3 [9][c], b3 [1]; every section starts on a multiple of 4 floats
struct PredParams { int w1, b1, w2, b2, w3, b3, total; };
VP_BE_HD PredParams pred_params(int c) {
  PredParams p;
  p.w1 = 0;
  p.b1 = p.w1 + rnd4(9 * c * 2 * c);
  p.w2 = p.b1 + rnd4(2 * c);
  p.b2 = p.w2 + rnd4(9 * 2 * c * c);
  p.w3 = p.b2 + rnd4(c);
  p.b3 = p.w3 + rnd4(9 * c);
  p.total = p.b3 + 4;
  return p;
}

// element i of an Up block's packed parameters from the reference-layout tensors: w1 (cmid, cin + 2, 3, 3), w2 (cmid, cmid, 3, 3) and
// each BatchNorm's gamma, beta, running mean and variance.  s = gamma / sqrt(var + eps) and t = beta - mean s are formed in fp64
// (bn_fold_kernel's arithmetic); the scale goes INTO the weight -- the fp64 product w s is rounded once -- and t starts the sum.
struct BnRef { const float *gamma, *beta, *mean, *var; };
VP_BE_HD double bn_scale(const BnRef& bn, int n, double eps) { return (double)bn.gamma[n] / __builtin_sqrt((double)bn.var[n] + eps); }
VP_BE_HD float bn_shift(const BnRef& bn, int n, double eps) { return (float)((double)bn.beta[n] - (double)bn.mean[n] * bn_scale(bn, n, eps)); }

VP_BE_HD float up_pack_elem(int i, const float* w1, BnRef bn1, const float* w2, BnRef bn2, double eps, int cin, int cmid) {
  const UpParams P = up_params(cin, cmid);
  const int k1 = cin + 2;
  if (i < P.t1) {
    const int n = i % cmid, k = (i / cmid) % k1, tap = i / (cmid * k1);
    return (float)((double)w1[((size_t)n * k1 + k) * 9 + tap] * bn_scale(bn1, n, eps));
  }
  if (i < P.w2) {
    const int n = i - P.t1;
    return n < cmid ? bn_shift(bn1, n, eps) : 0.f;
  }
  if (i < P.t2) {
    const int j = i - P.w2;
    if (j >= 9 * cmid * cmid) return 0.f;
    const int n = j % cmid, k = (j / cmid) % cmid, tap = j / (cmid * cmid);
    return (float)((double)w2[((size_t)n * cmid + k) * 9 + tap] * bn_scale(bn2, n, eps));
  }
  const int n = i - P.t2;
  return n < cmid ? bn_shift(bn2, n, eps) : 0.f;
}

// element i of a predictor's packed parameters from w1 (2c, c, 3, 3), b1, w2 (c, 2c, 3, 3), b2, w3 (1, c, 3, 3), b3
VP_BE_HD float pred_pack_elem(int i, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                              int c) {
  const PredParams P = pred_params(c);
  const int c2 = 2 * c;
  if (i < P.b1) {
    if (i >= 9 * c * c2) return 0.f;
    const int n = i % c2, k = (i / c2) % c, tap = i / (c2 * c);
    return w1[((size_t)n * c + k) * 9 + tap];
  }
  if (i < P.w2) return i - P.b1 < c2 ? b1[i - P.b1] : 0.f;
  if (i < P.b2) {
    const int j = i - P.w2;
    if (j >= 9 * c2 * c) return 0.f;
    const int n = j % c, k = (j / c) % c2, tap = j / (c * c2);
    return w2[((size_t)n * c2 + k) * 9 + tap];
  }
  if (i < P.w3) return i - P.b2 < c ? b2[i - P.b2] : 0.f;
  if (i < P.b3) {
    const int j = i - P.w3;
    if (j >= 9 * c) return 0.f;
    const int k = j % c, tap = j / c;
    return w3[(size_t)k * 9 + tap];
  }
  return i == P.b3 ? b3[0] : 0.f;
}

// ---- staging ------------------------------------------------------------------------------------------------------------------------
// channels [k0, k0 + cs) of the XH x XW halo tile of one image x [H][W][C] -> xs [pixel][ps]; 0 outside the image
template <int TSTEP>
VP_BE_HD void stage_halo(float* xs, const float* x, int H, int W, int C, int k0, int cs, int ps, int h0, int w0, int tid0) {
  if ((cs & 3) == 0) {
    const int q = cs >> 2;
    for (int t = tid0; t < NT; t += TSTEP)
      for (int idx = t; idx < XH * XW * q; idx += NT) {
        const int pix = idx / q, ch = (idx - pix * q) * 4;
        const int r = pix / XW, c = pix - r * XW, h = h0 - 3 + r, w = w0 - 3 + c;
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (inside(h, w, H, W)) v = *reinterpret_cast<const f4*>(x + ((size_t)h * W + w) * C + k0 + ch);
        *reinterpret_cast<f4*>(xs + pix * ps + ch) = v;
      }
  } else {
    for (int t = tid0; t < NT; t += TSTEP)
      for (int idx = t; idx < XH * XW * cs; idx += NT) {
        const int pix = idx / cs, ch = idx - pix * cs;
        const int r = pix / XW, c = pix - r * XW, h = h0 - 3 + r, w = w0 - 3 + c;
        xs[pix * ps + ch] = inside(h, w, H, W) ? x[((size_t)h * W + w) * C + k0 + ch] : 0.f;
      }
  }
}

template <int TSTEP>
VP_BE_HD void stage_copy(float* dst, const float* src, int n, int tid0) {
  for (int t = tid0; t < NT; t += TSTEP)
    for (int i = t; i < n; i += NT) dst[i] = src[i];
}

// ---- 3 x 3 convolution of one output pixel over an LDS region -------------------------------------------------------------------------
// acc[n] += sum over tap (dr, dc) and k < K of in[(r + dr, c + dc)][k] * w[tap][k][n]: (r, c) are the output pixel's coordinates in
// its own region, whose origin lies one pixel inside the input region's (iw = the input region's width, ps its pixel stride).
// Every lane of a wave reads the same weight address (an LDS broadcast); the traffic that matters is one 16-B read of x per four k.
template <int N>
VP_BE_HD void conv3_acc(float* acc, const float* in, int ps, int iw, int r, int c, const float* w, int K) {
  for (int tap = 0; tap < 9; ++tap) {
    const int dr = tap / 3, dc = tap - 3 * dr;
    const float* xp = in + ((r + dr) * iw + c + dc) * ps;
    const float* wp = w + tap * K * N;
    if ((K & 3) == 0) {
      for (int k = 0; k < K; k += 4) {
        const f4 xv = *reinterpret_cast<const f4*>(xp + k);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float* wk = wp + (k + u) * N;
          if constexpr ((N & 3) == 0) {
#pragma unroll
            for (int n = 0; n < N; n += 4) {
              const f4 wv = *reinterpret_cast<const f4*>(wk + n);
              acc[n] = __builtin_fmaf(xv[u], wv[0], acc[n]);
              acc[n + 1] = __builtin_fmaf(xv[u], wv[1], acc[n + 1]);
              acc[n + 2] = __builtin_fmaf(xv[u], wv[2], acc[n + 2]);
              acc[n + 3] = __builtin_fmaf(xv[u], wv[3], acc[n + 3]);
            }
          } else {
#pragma unroll
            for (int n = 0; n < N; ++n) acc[n] = __builtin_fmaf(xv[u], wk[n], acc[n]);
          }
        }
      }
    } else {
      for (int k = 0; k < K; ++k) {
        const float xv = xp[k];
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = __builtin_fmaf(xv, wp[k * N + n], acc[n]);
      }
    }
  }
}

// ---- the Up block -----------------------------------------------------------------------------------------------------------------------
// LDS (floats): the input slice and, after the first convolution, region B in the same place; the slice's weights; the coordinate
// channels' weights; t1, W2, t2 as they lie in the parameter block; region A
struct UpLds { int xs, w1, wc, tail, a, total; };
VP_BE_HD UpLds up_lds(int cin, int cmid) {
  const int cs = cin < CS ? cin : CS;
  const UpParams P = up_params(cin, cmid);
  const int nx = XH * XW * pix_stride(cs), nb = BH * BW * pix_stride(cmid);
  UpLds L;
  L.xs = 0;
  L.w1 = rnd4(nx > nb ? nx : nb);
  L.wc = L.w1 + 9 * cs * cmid;
  L.tail = L.wc + rnd4(9 * 2 * cmid);
  L.a = L.tail + (P.total - P.t1);
  L.total = L.a + rnd4(AH * AW * pix_stride(cmid));
  return L;
}

// x: one image [H][W][cin] of the head's input; p: the head's parameter block; y: the head's output image [2H][2W][CMID];
// acc: the CMID accumulators of each thread this call stands for (one row on the device, NT rows on the host)
template <int CMID, int TSTEP>
VP_BE_HD void up_tile(float* lds, const float* x, const float* p, float* y, int H, int W, int cin, int h0, int w0, int tid0,
                      float (*acc)[CMID]) {
  const int cs = cin < CS ? cin : CS, k1 = cin + 2;
  const UpParams P = up_params(cin, CMID);
  const UpLds L = up_lds(cin, CMID);
  const int psx = pix_stride(cs), psa = pix_stride(CMID);
  float* xs = lds + L.xs;
  float* w1s = lds + L.w1;
  float* wc = lds + L.wc;
  const float* t1 = lds + L.tail;
  const float* w2 = t1 + (P.w2 - P.t1);
  const float* t2 = t1 + (P.t2 - P.t1);
  float* ra = lds + L.a;
  float* rb = lds + L.xs;

  stage_copy<TSTEP>(lds + L.tail, p + P.t1, P.total - P.t1, tid0);
  for (int t = tid0; t < NT; t += TSTEP) {
    for (int i = t; i < 9 * 2 * CMID; i += NT) {                // [tap][column | row][n]
      const int n = i % CMID, j = (i / CMID) % 2, tap = i / (2 * CMID);
      wc[i] = p[P.w1 + (tap * k1 + cin + j) * CMID + n];
    }
#pragma unroll
    for (int n = 0; n < CMID; ++n) acc[TSTEP == 1 ? t : 0][n] = 0.f;
  }
  // the first convolution's cin image channels, CS at a time: the accumulators stay in registers across the slices
  for (int k0 = 0; k0 < cin; k0 += cs) {
    stage_halo<TSTEP>(xs, x, H, W, cin, k0, cs, psx, h0, w0, tid0);
    for (int t = tid0; t < NT; t += TSTEP)
      for (int i = t; i < 9 * cs * CMID; i += NT) {               // [tap][k][n] of this slice
        const int n = i % CMID, k = (i / CMID) % cs, tap = i / (CMID * cs);
        w1s[i] = p[P.w1 + (tap * k1 + k0 + k) * CMID + n];
      }
    tile_sync();
    for (int t = tid0; t < NT; t += TSTEP)
      if (t < AH * AW) conv3_acc<CMID>(acc[TSTEP == 1 ? t : 0], xs, psx, XW, t / AW, t % AW, w1s, cs);
    tile_sync();
  }
  // ... its two coordinate channels from the tap's position, the shift, ReLU; 0 outside the image -> A
  for (int t = tid0; t < NT; t += TSTEP)
    if (t < AH * AW) {
      const int h = h0 - 2 + t / AW, w = w0 - 2 + t % AW;
      float* v = acc[TSTEP == 1 ? t : 0];
      if (inside(h, w, H, W)) {
        for (int tap = 0; tap < 9; ++tap) {
          const int hh = h + tap / 3 - 1, ww = w + tap % 3 - 1;
          if (!inside(hh, ww, H, W)) continue;                    // the padding ring: the coordinate channels are 0 there
          const float fc = (float)ww, fr = (float)hh;
#pragma unroll
          for (int n = 0; n < CMID; ++n) v[n] = __builtin_fmaf(fr, wc[(tap * 2 + 1) * CMID + n], __builtin_fmaf(fc, wc[tap * 2 * CMID + n], v[n]));
        }
#pragma unroll
        for (int n = 0; n < CMID; ++n) {
          const float s = v[n] + t1[n];
          ra[t * psa + n] = s > 0.f ? s : 0.f;
        }
      } else {
#pragma unroll
        for (int n = 0; n < CMID; ++n) ra[t * psa + n] = 0.f;
      }
    }
  tile_sync();
  // the second convolution -> B (the input slice is dead).  Positions outside the image are computed but never read: the resize clamps.
  for (int t = tid0; t < NT; t += TSTEP)
    if (t < BH * BW) {
      float v[CMID];
#pragma unroll
      for (int n = 0; n < CMID; ++n) v[n] = t2[n];
      conv3_acc<CMID>(v, ra, psa, AW, t / BW, t % BW, w2, CMID);
#pragma unroll
      for (int n = 0; n < CMID; ++n) rb[t * psa + n] = v[n] > 0.f ? v[n] : 0.f;
    }
  tile_sync();
  // F.interpolate(scale_factor=2, mode="bilinear", align_corners=False): out[2i] = 0.25 in[i - 1] + 0.75 in[i],
  // out[2i + 1] = 0.75 in[i] + 0.25 in[i + 1], the source index clamped to the image
  const int H2 = 2 * H, W2 = 2 * W;
  for (int t = tid0; t < NT; t += TSTEP)
    for (int e = t; e < 2 * TH * 2 * TW * CMID; e += NT) {
      const int n = e % CMID, pc = (e / CMID) % (2 * TW), pr = e / (CMID * 2 * TW);
      const int oh = 2 * h0 + pr, ow = 2 * w0 + pc;
      if (oh >= H2 || ow >= W2) continue;
      int i0 = (oh >> 1) - 1 + (oh & 1), j0 = (ow >> 1) - 1 + (ow & 1);
      int i1 = i0 + 1, j1 = j0 + 1;
      const float a0 = (oh & 1) ? 0.75f : 0.25f, b0 = (ow & 1) ? 0.75f : 0.25f;
      i0 = i0 < 0 ? 0 : i0; j0 = j0 < 0 ? 0 : j0;
      i1 = i1 > H - 1 ? H - 1 : i1; j1 = j1 > W - 1 ? W - 1 : j1;
      const float* r0 = rb + (i0 - h0 + 1) * BW * psa + n;
      const float* r1 = rb + (i1 - h0 + 1) * BW * psa + n;
      const int c0 = (j0 - w0 + 1) * psa, c1 = (j1 - w0 + 1) * psa;
      const float top = b0 * r0[c0] + (1.f - b0) * r0[c1], bot = b0 * r1[c0] + (1.f - b0) * r1[c1];
      y[((size_t)oh * W2 + ow) * CMID + n] = a0 * top + (1.f - a0) * bot;
    }
}

// ---- the predictor ------------------------------------------------------------------------------------------------------------------------
// LDS (floats): the input tile and, after the first convolution, region B in the same place; the parameter block as it lies in
// global memory; region A
struct PredLds { int xs, p, a, total; };
VP_BE_HD PredLds pred_lds(int c) {
  const int nx = XH * XW * pix_stride(c), nb = BH * BW * pix_stride(c);
  PredLds L;
  L.xs = 0;
  L.p = rnd4(nx > nb ? nx : nb);
  L.a = L.p + pred_params(c).total;
  L.total = L.a + rnd4(AH * AW * pix_stride(2 * c));
  return L;
}

// x: one image [H][W][C]; p: the head's parameter block; logits / mask: the head's output image [H][W] (mask may be null:
// mask = logit >= threshold, the reference's post-processing of the raw output, test_BE.py:35-39)
template <int C, int TSTEP>
VP_BE_HD void pred_tile(float* lds, const float* x, const float* p, float* logits, unsigned char* mask, float threshold, int H, int W,
                        int h0, int w0, int tid0) {
  constexpr int C2 = 2 * C;
  const PredParams P = pred_params(C);
  const PredLds L = pred_lds(C);
  const int psx = pix_stride(C), psa = pix_stride(C2);
  float* xs = lds + L.xs;
  const float* q = lds + L.p;
  float* ra = lds + L.a;
  float* rb = lds + L.xs;
  stage_copy<TSTEP>(lds + L.p, p, P.total, tid0);
  stage_halo<TSTEP>(xs, x, H, W, C, 0, C, psx, h0, w0, tid0);
  tile_sync();
  for (int t = tid0; t < NT; t += TSTEP)
    if (t < AH * AW) {
      const bool in = inside(h0 - 2 + t / AW, w0 - 2 + t % AW, H, W);
      float v[C2];
#pragma unroll
      for (int n = 0; n < C2; ++n) v[n] = q[P.b1 + n];
      if (in) conv3_acc<C2>(v, xs, psx, XW, t / AW, t % AW, q + P.w1, C);
#pragma unroll
      for (int n = 0; n < C2; ++n) ra[t * psa + n] = in ? v[n] : 0.f;       // 0 outside the image, not the bias
    }
  tile_sync();
  for (int t = tid0; t < NT; t += TSTEP)
    if (t < BH * BW) {
      const bool in = inside(h0 - 1 + t / BW, w0 - 1 + t % BW, H, W);
      float v[C];
#pragma unroll
      for (int n = 0; n < C; ++n) v[n] = q[P.b2 + n];
      if (in) conv3_acc<C>(v, ra, psa, AW, t / BW, t % BW, q + P.w2, C2);
#pragma unroll
      for (int n = 0; n < C; ++n) rb[t * psx + n] = in ? v[n] : 0.f;
    }
  tile_sync();
  for (int t = tid0; t < NT; t += TSTEP)
    if (t < TH * TW) {
      const int h = h0 + t / TW, w = w0 + t % TW;
      if (h < H && w < W) {
        float v[1] = {q[P.b3]};
        conv3_acc<1>(v, rb, psx, BW, t / TW, t % TW, q + P.w3, C);
        logits[(size_t)h * W + w] = v[0];
        if (mask) mask[(size_t)h * W + w] = v[0] >= threshold ? 1 : 0;
      }
    }
}

}  // namespace be
}  // namespace vp
