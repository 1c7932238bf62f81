// Fused inference of the Style-GAN row (models/network_Style_GAN.py Generator / StyleEncoder / Discriminator under torch.no_grad(),
// train_Style_GAN.py:148-153,279-280), exact fp32 on NHWC.  Three kernels that the existing entries do not cover:
//   * scse2: relu?(SCSE_b(SCSE_a(x))), the tail of StyleUp.cat_convs, in two passes over x where two vp_scse_fwd_f32 calls read the
//     full-size tensor four times and write it twice.  Block a's spatial gate s_a[p] = sigmoid(w_sa . x[p,:] + b_sa) needs no pooling,
//     so block b's pooled input is known after ONE read of x:
//       mean_p y_a[.,ch] = c_a[ch] mean_p x[.,ch] + mean_p (x[.,ch] s_a[.])
//     pass 1 (read x): per chunk and channel sum x and sum x s_a;  gate (one workgroup per image): c_a, block b's pooled input, c_b;
//     pass 2 (read x, write y): s_a again, y_a = x (c_a + s_a), s_b from y_a in registers, y = y_a (c_b + s_b) [ReLU] [+ bf16 planes].
//     Thread map, chunk plan, float4 / scalar paths and ranges are scse.hip's (scse.h); none of the backward's leftovers is written.
//     Sums run in a fixed order without atomics: two runs give the same bits.
//   * cat2: the channel concatenation of two images, each NCHW or NHWC, as one NHWC tensor (the generator's and the discriminator's input).
//   * sg_out_tanh: final.3 + tanh, Conv2d(C, 3, 3) + bias + tanh over an NHWC map written as the NCHW result, after font_pred_kernel.
// DESIGN.md 17.1.
#include "scse.h"
#include "split.h"

namespace vp {
namespace {

// workspace of scse2, in floats: the two partial planes of pass 1, then the two channel gates
struct Scse2Ws {
  size_t px, pxs, ca, cb, total;
};
inline Scse2Ws scse2_ws(int B, int C, int nchunk) {
  Scse2Ws w;
  const size_t part = (size_t)B * nchunk * C;
  w.px = 0;
  w.pxs = part;
  w.ca = 2 * part;
  w.cb = w.ca + (size_t)B * C;
  w.total = w.cb + (size_t)B * C;
  return w;
}

// ---- pass 1: per chunk and channel, sum_p x and sum_p x s_a ---------------------------------------------------------------------------
template <typename T, int G, int K>
__global__ void __launch_bounds__(256) scse2_pool_kernel(const float* __restrict__ x, const float* __restrict__ wsa,
                                                         const float* __restrict__ bsa, float* __restrict__ part_x,
                                                         float* __restrict__ part_xs, int HW, int C, int ppc) {
  constexpr int S = 256 / G, W = sizeof(T) / 4, U = 2;
  __shared__ T sh_x[S][G * K], sh_s[S][G * K];
  const int b = blockIdx.y, chunk = blockIdx.x, j = threadIdx.x % G, slot = threadIdx.x / G, nel = C / W;
  const int p0 = chunk * ppc, p1 = min(HW, p0 + ppc);
  const T* xb = reinterpret_cast<const T*>(x + (size_t)b * HW * C);
  const T* wv = reinterpret_cast<const T*>(wsa);
  T w[K], a_x[K], a_s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = j + k * G;
    zero(w[k]);
    zero(a_x[k]);
    zero(a_s[k]);
    if (e < nel) w[k] = wv[e];
  }
  const float bsv = bsa[0];
  // the trip count depends on the chunk alone, so all 64 lanes of a wavefront reach every shuffle
  for (int q = p0; q < p1; q += S * U) {
    T v[U][K];
    float d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = q + u * S + slot;
      d[u] = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int e = j + k * G;
        zero(v[u][k]);
        if (p < p1 && e < nel) v[u][k] = xb[(size_t)p * nel + e];
        d[u] += dot(v[u][k], w[k]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float s = sigmoidf(slot_sum<G>(d[u]) + bsv);      // a pixel past the chunk was read as 0: it adds 0 to both sums
#pragma unroll
      for (int k = 0; k < K; ++k) {
        a_x[k] = add(a_x[k], v[u][k]);
        a_s[k] = add(a_s[k], muls(v[u][k], s));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    sh_x[slot][k * G + j] = a_x[k];
    sh_s[slot][k * G + j] = a_s[k];
  }
  __syncthreads();
  if (slot == 0) {
    const size_t row = ((size_t)b * gridDim.x + chunk) * C;
    T* ox = reinterpret_cast<T*>(part_x + row);
    T* os = reinterpret_cast<T*>(part_xs + row);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = j + k * G;
      if (e >= nel) continue;
      T t = sh_x[0][k * G + j], r = sh_s[0][k * G + j];
      for (int s = 1; s < S; ++s) {
        t = add(t, sh_x[s][k * G + j]);
        r = add(r, sh_s[s][k * G + j]);
      }
      ox[e] = t;
      os[e] = r;
    }
  }
}

// sigmoid(W2 relu(W1 pool + b1) + b2) of one image: pool [C] in LDS, hid [Cr] scratch in LDS, the gate to LDS and to global memory
__device__ __forceinline__ void scse2_channel_gate(const float* pool, float* hid, float* gate_lds, float* __restrict__ gate_out,
                                                   const float* __restrict__ w1, const float* __restrict__ b1,
                                                   const float* __restrict__ w2, const float* __restrict__ b2, int C, int Cr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int h = wave; h < Cr; h += 4) {
    float a = 0.f;
    for (int c = lane; c < C; c += 64) a += w1[(size_t)h * C + c] * pool[c];
    a = fmaxf(wave_sum(a) + b1[h], 0.f);
    if (lane == 0) hid[h] = a;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float a = b2[c];
    for (int h = 0; h < Cr; ++h) a += w2[(size_t)c * Cr + h] * hid[h];
    a = sigmoidf(a);
    gate_lds[c] = a;
    gate_out[c] = a;
  }
  __syncthreads();
}

// ---- the gates, one workgroup per image: c_a, block b's pooled input c_a mean(x) + mean(x s_a), c_b ------------------------------------
__global__ void __launch_bounds__(256) scse2_gate_kernel(const float* __restrict__ part_x, const float* __restrict__ part_xs,
                                                         const float* __restrict__ w1a, const float* __restrict__ b1a,
                                                         const float* __restrict__ w2a, const float* __restrict__ b2a,
                                                         const float* __restrict__ w1b, const float* __restrict__ b1b,
                                                         const float* __restrict__ w2b, const float* __restrict__ b2b,
                                                         float* __restrict__ ca, float* __restrict__ cb, int HW, int C, int Cr, int nchunk) {
  __shared__ float mx[kScseMaxC], mxs[kScseMaxC], gate[kScseMaxC], hid[kScseMaxC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float inv = 1.f / (float)HW;
  for (int c = tid; c < C; c += 256) {
    const float* px = part_x + (size_t)b * nchunk * C + c;
    const float* ps = part_xs + (size_t)b * nchunk * C + c;
    float a = 0.f, r = 0.f;
#pragma unroll 8
    for (int k = 0; k < nchunk; ++k) {
      a += px[(size_t)k * C];
      r += ps[(size_t)k * C];
    }
    mx[c] = a * inv;
    mxs[c] = r * inv;
  }
  __syncthreads();
  scse2_channel_gate(mx, hid, gate, ca + (size_t)b * C, w1a, b1a, w2a, b2a, C, Cr);
  for (int c = tid; c < C; c += 256) mx[c] = gate[c] * mx[c] + mxs[c];
  __syncthreads();
  scse2_channel_gate(mx, hid, gate, cb + (size_t)b * C, w1b, b1b, w2b, b2b, C, Cr);
}

// ---- pass 2: y = y_a (c_b + s_b) with y_a = x (c_a + s_a), both spatial gates formed in registers ----------------------------------------
template <typename T, int G, int K>
__global__ void __launch_bounds__(256) scse2_apply_kernel(const float* __restrict__ x, const float* __restrict__ ca,
                                                          const float* __restrict__ cb, const float* __restrict__ wsa,
                                                          const float* __restrict__ bsa, const float* __restrict__ wsb,
                                                          const float* __restrict__ bsb, float* __restrict__ y,
                                                          u16_t* __restrict__ y_split, size_t plane, int HW, int C, int ppc, int do_relu) {
  constexpr int S = 256 / G, W = sizeof(T) / 4, U = 2;
  const int b = blockIdx.y, j = threadIdx.x % G, slot = threadIdx.x / G, nel = C / W;
  const int p0 = blockIdx.x * ppc, p1 = min(HW, p0 + ppc);
  const size_t img = (size_t)b * HW * C;
  const T* xb = reinterpret_cast<const T*>(x + img);
  T* yb = reinterpret_cast<T*>(y + img);
  const T* cav = reinterpret_cast<const T*>(ca + (size_t)b * C);
  const T* cbv = reinterpret_cast<const T*>(cb + (size_t)b * C);
  const T* wav = reinterpret_cast<const T*>(wsa);
  const T* wbv = reinterpret_cast<const T*>(wsb);
  T ga[K], gb[K], wa[K], wb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = j + k * G;
    zero(ga[k]);
    zero(gb[k]);
    zero(wa[k]);
    zero(wb[k]);
    if (e < nel) {
      ga[k] = cav[e];
      gb[k] = cbv[e];
      wa[k] = wav[e];
      wb[k] = wbv[e];
    }
  }
  const float bav = bsa[0], bbv = bsb[0];
  // the trip count depends on the chunk alone, so all 64 lanes of a wavefront reach every shuffle
  for (int q = p0; q < p1; q += S * U) {
    T v[U][K];
    float d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = q + u * S + slot;
      d[u] = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int e = j + k * G;
        zero(v[u][k]);
        if (p < p1 && e < nel) v[u][k] = xb[(size_t)p * nel + e];
        d[u] += dot(v[u][k], wa[k]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float sa = sigmoidf(slot_sum<G>(d[u]) + bav);
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        v[u][k] = mul(v[u][k], adds(ga[k], sa));           // y_a (0 in the lanes and pixels that were read as 0)
        t += dot(v[u][k], wb[k]);
      }
      d[u] = t;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = q + u * S + slot;
      const float sb = sigmoidf(slot_sum<G>(d[u]) + bbv);
      if (p >= p1) continue;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int e = j + k * G;
        if (e >= nel) continue;
        T o = mul(v[u][k], adds(gb[k], sb));
        if (do_relu) o = relu(o);
        yb[(size_t)p * nel + e] = o;
        if constexpr (W == 4) {
          if (y_split) store_split4(y_split, plane, img + (size_t)p * C + 4 * (size_t)e, o.x, o.y, o.z, o.w);
        }
      }
    }
  }
}

// ---- cat2: out[b][p][0..Ca) = a, out[b][p][Ca..Ca+Cb) = b; a source is [B][C][HW] (NCHW) or [B][HW][C] (NHWC) -------------------------
__global__ void sg_cat2_kernel(const float* __restrict__ a, int a_nhwc, const float* __restrict__ bsrc, int b_nhwc, float* __restrict__ out,
                               size_t n, int HW, int Ca, int Cb) {
  const int Ct = Ca + Cb;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % Ct);
    const size_t r = i / Ct;
    const int p = (int)(r % HW);
    const size_t img = r / HW;
    float v;
    if (c < Ca) v = a_nhwc ? a[(img * HW + p) * Ca + c] : a[(img * Ca + c) * HW + p];
    else v = b_nhwc ? bsrc[(img * HW + p) * Cb + (c - Ca)] : bsrc[(img * Cb + (c - Ca)) * HW + p];
    out[i] = v;
  }
}

// ---- final.3 + tanh: out[b][o][h][w] = tanh(bias[o] + sum_{tap, c} x[b][h + dh][w + dw][c] W[o][c][tap]), o = 0, 1, 2 ------------------
// LP lanes per pixel (4, 8 or 16: as many as C / 4 fills, so that no lane idles at C = 32), four channels per lane and trip; the taps
// in order within a lane, then the butterfly over the LP lanes; lanes 0, 1, 2 of the group store one output channel each.
constexpr int kSgOut = 3;
inline bool sg_out_supported(int C) { return C >= 4 && C <= 256 && C % 4 == 0; }
__host__ __device__ inline int sg_out_params_floats(int C) { return kSgOut * 9 * C + 4; }

template <int LP>
__global__ void __launch_bounds__(256) sg_out_tanh_kernel(const float* __restrict__ x, const float* __restrict__ par, float* __restrict__ out,
                                                          int B, int H, int W, int C) {
  const size_t npix = (size_t)B * H * W, hw = (size_t)H * W;
  const int sub = threadIdx.x % LP;
  const size_t first = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / LP, step = ((size_t)gridDim.x * blockDim.x) / LP;
  const size_t trips = (npix + step - 1) / step;        // every lane of a group runs the same trips: the shuffles stay converged
  for (size_t it = 0; it < trips; ++it) {
    const size_t pix = first + it * step;
    const bool live = pix < npix;
    const size_t pc = live ? pix : 0;
    const int w0 = (int)(pc % W), h0 = (int)((pc / W) % H);
    const size_t b = pc / hw;
    float s[kSgOut] = {0.f, 0.f, 0.f};
    for (int c = sub * 4; c < C; c += 4 * LP) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int h = h0 + tap / 3 - 1, w = w0 + tap % 3 - 1;
        if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
          const float4 xv = *reinterpret_cast<const float4*>(x + ((b * H + h) * W + w) * C + c);
#pragma unroll
          for (int o = 0; o < kSgOut; ++o) {
            const float4 wv = *reinterpret_cast<const float4*>(par + (size_t)(o * 9 + tap) * C + c);
            s[o] = fmaf(xv.x, wv.x, s[o]);
            s[o] = fmaf(xv.y, wv.y, s[o]);
            s[o] = fmaf(xv.z, wv.z, s[o]);
            s[o] = fmaf(xv.w, wv.w, s[o]);
          }
        }
      }
    }
#pragma unroll
    for (int o = 0; o < kSgOut; ++o)
#pragma unroll
      for (int off = LP / 2; off > 0; off >>= 1) s[o] += __shfl_xor(s[o], off, 64);
    if (live && sub < kSgOut) {
      const float v = (sub == 0 ? s[0] : (sub == 1 ? s[1] : s[2])) + par[kSgOut * 9 * C + sub];
      out[(b * kSgOut + sub) * hw + (pc - b * hw)] = tanhf(v);
    }
  }
}

// (3, C, 3, 3) -> [o][tap][C], then the three biases and a zero
__global__ void sg_out_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ params, int C) {
  const int n = sg_out_params_floats(C), nw = kSgOut * 9 * C;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (i < nw) {
      const int c = i % C, tap = (i / C) % 9, o = i / (9 * C);
      params[i] = w[((size_t)o * C + c) * 9 + tap];
    } else {
      params[i] = i - nw < kSgOut ? bias[i - nw] : 0.f;
    }
  }
}

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" {

size_t vp_scse2_workspace_bytes(int B, int HW, int C, int hidden) {
  if (B <= 0 || HW <= 0 || C <= 0 || hidden <= 0 || hidden > C) return 0;
  const ScsePlan pl = scse_plan(B, HW, C);
  return scse2_ws(B, C, pl.nchunk).total * sizeof(float);
}

// Host-only: where a plan should take vp_scse2_fwd_f32 over two vp_scse_fwd_f32 calls: the 16-byte path (it was faster at every shape
// measured, C = 64 .. 256: DESIGN.md 17.1; the scalar path was not measured).
int vp_scse2_preferred(int B, int HW, int C, int hidden) {
  return B > 0 && HW > 0 && hidden > 0 && hidden <= C && C > 0 && C <= kScseMaxC && C % 4 == 0 ? 1 : 0;
}

int vp_scse2_fwd_f32(const float* x, const float* w1a, const float* b1a, const float* w2a, const float* b2a, const float* w_sa,
                     const float* b_sa, const float* w1b, const float* b1b, const float* w2b, const float* b2b, const float* w_sb,
                     const float* b_sb, float* y, void* y_split, int B, int HW, int C, int hidden, int relu, void* ws, size_t ws_bytes,
                     vp_stream stream) {
  if (int rc = scse_check_dims("vp_scse2_fwd_f32", B, HW, C, hidden)) return rc;      // first: an empty hidden layer has null weights
  VP_REQUIRE(x && w1a && b1a && w2a && b2a && w_sa && b_sa && w1b && b1b && w2b && b2b && w_sb && b_sb && y && ws,
             "vp_scse2_fwd_f32: null pointer");
  const ScsePlan pl = scse_plan(B, HW, C);
  const Scse2Ws lay = scse2_ws(B, C, pl.nchunk);
  if (ws_bytes < lay.total * sizeof(float))
    return fail(VP_ERR_WORKSPACE, "vp_scse2_fwd_f32: workspace of %zu bytes, %zu needed", ws_bytes, lay.total * sizeof(float));
  const bool vec = C % 4 == 0 && aligned16(x, y, w_sa, w_sb) && aligned16((const float*)ws);
  if (int rc = scse_check_path("vp_scse2_fwd_f32", vec, C)) return rc;
  VP_REQUIRE(!y_split || (C % 8 == 0 && vec && aligned16((const float*)y_split)),
             "vp_scse2_fwd_f32: the bf16 planes need C %% 8 == 0 and 16-byte aligned tensors, planes and workspace");
  hipStream_t s = (hipStream_t)stream;
  float* f = (float*)ws;
  const dim3 grid(pl.nchunk, B), blk(256);
#define SCSE2_POOL(T, G, K) \
  hipLaunchKernelGGL((scse2_pool_kernel<T, G, K>), grid, blk, 0, s, x, w_sa, b_sa, f + lay.px, f + lay.pxs, HW, C, pl.ppc)
  if (vec) SCSE_DISPATCH(float4, C / 4, SCSE2_POOL);
  else SCSE_DISPATCH(float, C, SCSE2_POOL);
#undef SCSE2_POOL
  hipLaunchKernelGGL(scse2_gate_kernel, dim3(B), blk, 0, s, (const float*)(f + lay.px), (const float*)(f + lay.pxs), w1a, b1a, w2a, b2a, w1b,
                     b1b, w2b, b2b, f + lay.ca, f + lay.cb, HW, C, hidden, pl.nchunk);
  const size_t plane = (size_t)B * HW * C;
#define SCSE2_APPLY(T, G, K)                                                                                                          \
  hipLaunchKernelGGL((scse2_apply_kernel<T, G, K>), grid, blk, 0, s, x, (const float*)(f + lay.ca), (const float*)(f + lay.cb), w_sa, b_sa, \
                     w_sb, b_sb, y, (u16_t*)y_split, plane, HW, C, pl.ppc, relu)
  if (vec) SCSE_DISPATCH(float4, C / 4, SCSE2_APPLY);
  else SCSE_DISPATCH(float, C, SCSE2_APPLY);
#undef SCSE2_APPLY
  return check_launch("vp_scse2_fwd_f32");
}

int vp_cat2_nhwc_f32(const float* a, int a_nhwc, const float* b, int b_nhwc, float* out, int B, int HW, int Ca, int Cb, vp_stream stream) {
  VP_REQUIRE(a && b && out, "vp_cat2_nhwc_f32: null pointer");
  VP_REQUIRE(B > 0 && HW > 0 && Ca > 0 && Cb > 0 && (long long)Ca + Cb <= 0x7fffffffLL, "vp_cat2_nhwc_f32: sizes must be positive");
  const size_t n = (size_t)B * HW * ((size_t)Ca + Cb);
  return launch_flat("vp_cat2_nhwc_f32", sg_cat2_kernel, n, FLAT_CAP, (hipStream_t)stream, a, a_nhwc ? 1 : 0, b, b_nhwc ? 1 : 0, out, n, HW,
                     Ca, Cb);
}

size_t vp_sg_out_params_floats(int C) { return sg_out_supported(C) ? (size_t)sg_out_params_floats(C) : 0; }

// Host-only: where a plan should take vp_sg_out_tanh_f32 over convolution + tanh + transpose: C = 32, Generator.final's width and the
// one channel count it was measured at.
int vp_sg_out_tanh_preferred(int B, int H, int W, int C) { return B > 0 && H > 0 && W > 0 && C == 32 ? 1 : 0; }

int vp_sg_out_pack_f32(const float* w, const float* bias, float* params, int C, vp_stream stream) {
  VP_REQUIRE(w && bias && params, "vp_sg_out_pack_f32: null pointer");
  VP_REQUIRE(sg_out_supported(C), "vp_sg_out_pack_f32: C must be a multiple of 4, 4 <= C <= 256");
  hipLaunchKernelGGL(sg_out_pack_kernel, dim3((sg_out_params_floats(C) + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, bias, params, C);
  return check_launch("vp_sg_out_pack_f32");
}

int vp_sg_out_tanh_f32(const float* x, const float* params, float* out, int B, int H, int W, int C, vp_stream stream) {
  VP_REQUIRE(x && params && out, "vp_sg_out_tanh_f32: null pointer");
  VP_REQUIRE(sg_out_supported(C), "vp_sg_out_tanh_f32: C must be a multiple of 4, 4 <= C <= 256");
  VP_REQUIRE(B > 0 && H > 0 && W > 0, "vp_sg_out_tanh_f32: sizes must be positive");
  VP_REQUIRE(aligned16(x, params), "vp_sg_out_tanh_f32: x and params must be 16-byte aligned");
  const size_t npix = (size_t)B * H * W;
  hipStream_t s = (hipStream_t)stream;
#define SG_OUT(LP) hipLaunchKernelGGL(sg_out_tanh_kernel<LP>, dim3(grid_for(npix * LP, 256)), dim3(256), 0, s, x, params, out, B, H, W, C)
  if (C <= 16) SG_OUT(4);
  else if (C <= 32) SG_OUT(8);
  else SG_OUT(16);
#undef SG_OUT
  return check_launch("vp_sg_out_tanh_f32");
}

}  // extern "C"
