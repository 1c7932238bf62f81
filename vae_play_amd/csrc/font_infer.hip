// Fused eval-mode inference of the font U-Net (models/networks_BE_font.py ComposeNet, as test_BE_font.py runs it), exact fp32:
//   * conv_in_kernel: Conv2d(k, stride, bias=False) + InstanceNorm2d + activation in ONE launch for maps of at most 256 pixels.  A
//     workgroup owns 256 output rows = whole images and 16 output channels; the contraction runs on v_mfma_f32_16x16x4_f32 with K
//     streamed through LDS in slices of 32 (register-staged one slice ahead, as igemm.h does); the epilogue computes each image's
//     per-channel mean and CENTRED variance from the resident accumulators and writes act((acc - mean) * rstd) once;
//   * font_pred_kernel: the two heads' Conv2d(C, 1, 3) + bias in one launch, with the thresholded masks;
//   * the relay_convs.0 input row and the 1 x 1 self-attention tail of the embedding branch.
// What the whole-image kernel takes is stated in font_infer.h; DESIGN.md 11.1.
#include "common.h"
#include "problems.h"
#include "font_infer.h"

namespace vp {

using namespace font;

typedef float f32x4acc __attribute__((ext_vector_type(4)));

constexpr int F_LDK = SLICE_K + 4;                  // LDS row stride in floats: 16 lanes of a ds_read_b128 group on 64 distinct banks
constexpr int A_ROWS_PER_THREAD = TILE_ROWS / 32;   // 16-byte loads of the activation tile per thread and K slice

__device__ __forceinline__ float font_act(float v, int act, float slope) {
  if (act == VP_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == VP_ACT_LRELU) return v > 0.f ? v : v * slope;
  return v;
}

// Accumulator map of v_mfma_f32_16x16x4_f32: register r of lane l is row 4 * (l >> 4) + r, column l & 15 of a 16 x 16 tile.  Wave w
// owns tile rows [64 w, 64 w + 64) as four such tiles; tile t of wave w covers rows 64 w + 16 t ... + 15.  With P pixels per image:
//   P = 16: an image is one MFMA tile (four images per wave);  P = 64: a wave's four tiles;  P = 256: the four waves' sixteen tiles.
// An image's sum is formed the same way in every slot: the lane's registers in order, the four lane groups by two butterflies (both
// operands of each addition are the same pair of numbers in every lane, so every lane holds the same bits), the four waves as
// (w0 + w1) + (w2 + w3).  Nothing depends on which slot or tile the image sits in.
template <int P>
__device__ __forceinline__ float image_sum(const float (&v)[16], int g, float* red, int wave, int col) {
  constexpr int NG = P >= 64 ? 1 : 64 / P;   // images per wave
  constexpr int RG = 16 / NG;                // accumulator registers per image and lane
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < RG; ++q) s += v[g * RG + q];
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  if constexpr (P == 256) {
    __syncthreads();                         // (the previous use of red is over)
    if ((threadIdx.x & 63) < 16) red[wave * TILE_CH + col] = s;
    __syncthreads();
    s = (red[col] + red[TILE_CH + col]) + (red[2 * TILE_CH + col] + red[3 * TILE_CH + col]);
  }
  return s;
}

template <int P>
__global__ void __launch_bounds__(256) conv_in_kernel(const float* __restrict__ x, const float* __restrict__ wp, float* __restrict__ y,
                                                      int ldy, int B, int H, int W, int Wo, int Cin, int ks, int stride, float eps,
                                                      int act, float slope) {
  __shared__ __attribute__((aligned(16))) float lds[(TILE_ROWS + TILE_CH) * F_LDK];
  __shared__ float red[4 * TILE_CH];
  float* As = lds;
  float* Bs = lds + TILE_ROWS * F_LDK;
  constexpr int G = TILE_ROWS / P;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, lg = lane >> 4;
  const int img0 = blockIdx.x * G, n0 = blockIdx.y * TILE_CH;
  const int pad = (ks - 1) / 2, K = ks * ks * Cin, nk = K / SLICE_K;
  const int kc = (tid & 7) * 4, r0 = tid >> 3;

  // the rows this thread stages: output pixel -> top-left input pixel; a slot past the batch never passes the bounds test
  int ih0[A_ROWS_PER_THREAD], iw0[A_ROWS_PER_THREAD], bi[A_ROWS_PER_THREAD];
#pragma unroll
  for (int i = 0; i < A_ROWS_PER_THREAD; ++i) {
    const int m = r0 + 32 * i;
    const int b = img0 + m / P, p = m % P;
    const bool live = b < B;
    bi[i] = live ? b : 0;
    ih0[i] = live ? (p / Wo) * stride - pad : -(1 << 20);
    iw0[i] = (p % Wo) * stride - pad;
  }
  const bool stages_b = tid < TILE_CH * 8;
  const float* wrow = wp + (size_t)(n0 + (stages_b ? r0 : 0)) * K + kc;

  vp_f32x4 sa[A_ROWS_PER_THREAD], sb;
  auto stage_load = [&](int k0) {
    const int tap = k0 / Cin, c = k0 - tap * Cin + kc;
    const int kh = tap / ks, kw = tap - kh * ks;
#pragma unroll
    for (int i = 0; i < A_ROWS_PER_THREAD; ++i) {
      const int ih = ih0[i] + kh, iw = iw0[i] + kw;
      const bool in = (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
      sa[i] = in ? *reinterpret_cast<const vp_f32x4*>(x + (((size_t)bi[i] * H + ih) * W + iw) * Cin + c) : vp_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (stages_b) sb = *reinterpret_cast<const vp_f32x4*>(wrow + k0);
  };
  auto stage_write = [&]() {
#pragma unroll
    for (int i = 0; i < A_ROWS_PER_THREAD; ++i) *reinterpret_cast<vp_f32x4*>(&As[(r0 + 32 * i) * F_LDK + kc]) = sa[i];
    if (stages_b) *reinterpret_cast<vp_f32x4*>(&Bs[r0 * F_LDK + kc]) = sb;
  };

  f32x4acc acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4acc{0.f, 0.f, 0.f, 0.f};

  stage_load(0);
  stage_write();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    if (more) stage_load((kt + 1) * SLICE_K);
    // lane group lg takes k = 16 blk + 4 lg + j at MFMA step j, the same permutation for both operands: one ds_read_b128 feeds four steps
#pragma unroll
    for (int blk = 0; blk < SLICE_K / 16; ++blk) {
      vp_f32x4 a[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) a[t] = *reinterpret_cast<const vp_f32x4*>(&As[(wave * 64 + 16 * t + col) * F_LDK + blk * 16 + lg * 4]);
      const vp_f32x4 b = *reinterpret_cast<const vp_f32x4*>(&Bs[col * F_LDK + blk * 16 + lg * 4]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], b[j], acc[t], 0, 0, 0);
    }
    __syncthreads();
    if (more) {
      stage_write();
      __syncthreads();
    }
  }

  // ---- epilogue: per (image, channel) statistics from the accumulators, normalise, activate, store ----
  float v[16];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[4 * t + r] = acc[t][r];
  constexpr int NG = P >= 64 ? 1 : 64 / P, RG = 16 / NG;
  constexpr float inv_p = 1.f / (float)P;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const float mean = image_sum<P>(v, g, red, wave, col) * inv_p;
    float d[16];
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      const float dev = v[g * RG + q] - mean;
      v[g * RG + q] = dev;
      d[g * RG + q] = dev * dev;
    }
    const float var = image_sum<P>(d, g, red, wave, col) * inv_p;
    const float rstd = 1.f / sqrtf(var + eps);
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      const int idx = g * RG + q;
      const int m = wave * 64 + 16 * (idx >> 2) + 4 * lg + (idx & 3);
      const int b = img0 + m / P, p = m % P;
      if (b < B) y[((size_t)b * P + p) * ldy + n0 + col] = font_act(v[idx] * rstd, act, slope);
    }
  }
}

// wp[n][tap][c] = w[n][c][tap]: the contraction's K order (tap-major, channel contiguous)
__global__ void conv_in_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin, int taps) {
  const size_t n = (size_t)Cout * Cin * taps;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cin);
    const size_t r = i / Cin;
    const int tap = (int)(r % taps);
    const size_t co = r / taps;
    wp[i] = w[(co * Cin + c) * taps + tap];
  }
}

// ---- the heads' output stage: logits[head][b][h][w] = bias + sum_{tap, c} x[head][b][h + dh][w + dw][c] W[c][tap] -------------------
// Sixteen lanes per pixel, four channels per lane and trip; the taps in order within a lane, then the butterfly over the sixteen lanes.
__global__ void __launch_bounds__(256) font_pred_kernel(const float* __restrict__ x, size_t x_head_stride, const float* __restrict__ params,
                                                        float* __restrict__ logits, unsigned char* __restrict__ mask, float threshold,
                                                        int B, int H, int W, int C) {
  const int head = blockIdx.y;
  const float* xh = x + head * x_head_stride;
  const float* par = params + (size_t)head * pred_params_floats(C);
  const size_t npix = (size_t)B * H * W;
  const int sub = threadIdx.x & 15;
  const size_t first = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4, step = ((size_t)gridDim.x * blockDim.x) >> 4;
  const size_t trips = (npix + step - 1) / step;        // every lane of a group runs the same trips: the shuffles stay converged
  for (size_t it = 0; it < trips; ++it) {
    const size_t pix = first + it * step;
    const bool live = pix < npix;
    const size_t pc = live ? pix : 0;
    const int w0 = (int)(pc % W), h0 = (int)((pc / W) % H);
    const size_t b = pc / ((size_t)W * H);
    float s = 0.f;
    for (int c = sub * 4; c < C; c += 64) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int h = h0 + tap / 3 - 1, w = w0 + tap % 3 - 1;
        if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
          const vp_f32x4 xv = *reinterpret_cast<const vp_f32x4*>(xh + ((b * H + h) * W + w) * C + c);
          const vp_f32x4 wv = *reinterpret_cast<const vp_f32x4*>(par + tap * C + c);
#pragma unroll
          for (int j = 0; j < 4; ++j) s = fmaf(xv[j], wv[j], s);
        }
      }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (live && sub == 0) {
      const float v = s + par[9 * C];
      logits[head * npix + pix] = v;
      if (mask) mask[head * npix + pix] = v >= threshold ? 1 : 0;
    }
  }
}

__global__ void font_pred_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ params, int C) {
  const int n = pred_params_floats(C);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (i < 9 * C) params[i] = w[(i % C) * 9 + i / C];          // (1, C, 3, 3) -> [tap][C]
    else params[i] = i == 9 * C ? bias[0] : 0.f;
  }
}

// ---- relay_convs.0's input row: [map flattened in (C, H, W) order | label | style] from the NHWC map ---------------------------------
__global__ void font_relay_input_kernel(const float* __restrict__ map, const float* __restrict__ label, const float* __restrict__ style,
                                        float* __restrict__ out, int B, int HW, int C, int E) {
  const int row = C * HW + 2 * E;
  const size_t n = (size_t)B * row;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / row;
    const int j = (int)(i - b * row);
    float v;
    if (j < C * HW) v = map[(b * HW + j % HW) * C + j / HW];
    else if (j < C * HW + E) v = label[b * E + (j - C * HW)];
    else v = style[b * E + (j - C * HW - E)];
    out[i] = v;
  }
}

// ---- SelfAttentionBlock on a 1 x 1 map (models/blocks.py:77-96): the softmax over one position is 1, so out = gamma relu(v) + x ------
// (out may be x: each element is read before it is written)
__global__ void font_attn1_kernel(const float* __restrict__ v_pre, const float* x, const float* __restrict__ gamma, float* out, size_t n) {
  const float g = gamma[0];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float v = v_pre[i];
    out[i] = g * (v > 0.f ? v : 0.f) + x[i];
  }
}

}  // namespace vp

using namespace vp;

extern "C" {

int vp_conv_in_supported(int H, int W, int Cin, int Cout, int ks, int stride) { return conv_in_supported(H, W, Cin, Cout, ks, stride) ? 1 : 0; }

int vp_conv_in_preferred(int H, int W, int Cin, int Cout, int ks, int stride) { return conv_in_preferred(H, W, Cin, Cout, ks, stride) ? 1 : 0; }

int vp_conv_in_pack_f32(const float* w_ref, float* w_packed, int Cout, int Cin, int ks, vp_stream stream) {
  VP_REQUIRE(w_ref && w_packed, "vp_conv_in_pack_f32: null pointer");
  VP_REQUIRE(Cout > 0 && Cin > 0 && (ks == 1 || ks == 3), "vp_conv_in_pack_f32: Cout, Cin > 0 and ks 1 | 3");
  return launch_flat("vp_conv_in_pack_f32", conv_in_pack_kernel, (size_t)Cout * Cin * ks * ks, FLAT_CAP, (hipStream_t)stream, w_ref,
                     w_packed, Cout, Cin, ks * ks);
}

int vp_conv_in_act_f32(const float* x, const float* w_packed, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int ks, int stride,
                       float eps, int act, float slope, vp_stream stream) {
  VP_REQUIRE(x && w_packed && y, "vp_conv_in_act_f32: null pointer");
  ConvInGeom g;
  VP_REQUIRE(conv_in_supported(H, W, Cin, Cout, ks, stride) && conv_in_geom(H, W, ks, stride, g),
             "vp_conv_in_act_f32: takes (ks, stride) (3,1) (3,2) (1,1), an output map of 16, 64 or 256 pixels, Cin and Cout multiples of 64 "
             "up to 1024 (vp_conv_in_supported)");
  VP_REQUIRE(B > 0 && ldy >= Cout && eps >= 0.f, "vp_conv_in_act_f32: B > 0, ldy >= Cout, eps >= 0");
  VP_REQUIRE(act == VP_ACT_NONE || act == VP_ACT_RELU || act == VP_ACT_LRELU, "vp_conv_in_act_f32: act none | relu | lrelu");
  VP_REQUIRE(aligned16(x, w_packed), "vp_conv_in_act_f32: x and w_packed must be 16-byte aligned");
  const long long tiles = ((long long)B + g.images - 1) / g.images;
  VP_REQUIRE(tiles <= 0x7fffffffLL, "vp_conv_in_act_f32: too many tiles");
  const dim3 grid((unsigned)tiles, Cout / TILE_CH);
  hipStream_t s = (hipStream_t)stream;
#define VP_CONV_IN(PP) \
  hipLaunchKernelGGL(conv_in_kernel<PP>, grid, dim3(256), 0, s, x, w_packed, y, ldy, B, H, W, g.Wo, Cin, ks, stride, eps, act, slope)
  switch (g.pixels) {
    case 16: VP_CONV_IN(16); break;
    case 64: VP_CONV_IN(64); break;
    default: VP_CONV_IN(256); break;
  }
#undef VP_CONV_IN
  return check_launch("vp_conv_in_act_f32");
}

size_t vp_font_pred_params_floats(int C) { return pred_supported(C) ? (size_t)pred_params_floats(C) : 0; }

int vp_font_pred_pack_f32(const float* w, const float* bias, float* params, int C, vp_stream stream) {
  VP_REQUIRE(w && bias && params, "vp_font_pred_pack_f32: null pointer");
  VP_REQUIRE(pred_supported(C), "vp_font_pred_pack_f32: C must be a multiple of 4, 4 <= C <= 256");
  hipLaunchKernelGGL(font_pred_pack_kernel, dim3((pred_params_floats(C) + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, bias, params, C);
  return check_launch("vp_font_pred_pack_f32");
}

int vp_font_pred_infer_f32(const float* x, size_t x_head_stride, const float* params, float* logits, unsigned char* mask, float threshold,
                           int heads, int B, int H, int W, int C, vp_stream stream) {
  VP_REQUIRE(x && params && logits, "vp_font_pred_infer_f32: null pointer");
  VP_REQUIRE(pred_supported(C), "vp_font_pred_infer_f32: C must be a multiple of 4, 4 <= C <= 256");
  VP_REQUIRE(heads > 0 && heads <= 65535 && B > 0 && H > 0 && W > 0, "vp_font_pred_infer_f32: sizes must be positive (heads <= 65535)");
  VP_REQUIRE(aligned16(x, params) && x_head_stride % 4 == 0, "vp_font_pred_infer_f32: operands must be 16-byte aligned");
  const size_t npix = (size_t)B * H * W;
  hipLaunchKernelGGL(font_pred_kernel, dim3(grid_for(npix * 16, 256), heads), dim3(256), 0, (hipStream_t)stream, x, x_head_stride, params,
                     logits, mask, threshold, B, H, W, C);
  return check_launch("vp_font_pred_infer_f32");
}

int vp_font_relay_input_f32(const float* map_nhwc, const float* label, const float* style, float* out, int B, int HW, int C, int E,
                            vp_stream stream) {
  VP_REQUIRE(map_nhwc && label && style && out, "vp_font_relay_input_f32: null pointer");
  VP_REQUIRE(B > 0 && HW > 0 && C > 0 && E > 0, "vp_font_relay_input_f32: sizes must be positive");
  VP_REQUIRE((long long)C * HW + 2LL * E <= 0x7fffffffLL, "vp_font_relay_input_f32: row too long");
  return launch_flat("vp_font_relay_input_f32", font_relay_input_kernel, (size_t)B * ((size_t)C * HW + 2 * (size_t)E), FLAT_CAP,
                     (hipStream_t)stream, map_nhwc, label, style, out, B, HW, C, E);
}

int vp_font_attn1_f32(const float* v_pre, const float* x, const float* gamma, float* out, size_t n, vp_stream stream) {
  VP_REQUIRE(v_pre && x && gamma && out && n > 0, "vp_font_attn1_f32: bad arguments");
  return launch_flat("vp_font_attn1_f32", font_attn1_kernel, n, FLAT_CAP, (hipStream_t)stream, v_pre, x, gamma, out, n);
}

}  // extern "C"
