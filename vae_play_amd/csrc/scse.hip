// SCSEBlock (models/blocks.py:52-65), forward and backward, fp32 on NHWC:
//   y = x * (c + s),   c[b,ch] = sigmoid(W2 relu(W1 mean_hw(x) + b1) + b2),   s[b,p] = sigmoid(sum_ch w_s[ch] x[b,p,ch] + b_s)
// optionally followed by the ReLU that ends StyleUp.cat_convs (models/network_Style_GAN.py:54-59), applied in the same store.
//
// The block is memory traffic and nothing else, so the kernels are organised around passes over the full-size tensor:
//   forward   pool (read x) -> gate (tiny) -> apply (read x, write y)                                    3 passes
//   backward  main (read x, dy, write dx) -> gate (tiny) -> params (tiny) -> final (dx += dpool / HW)    5 passes
// Every image is cut into chunks of whole pixels (scse_plan), one workgroup per (chunk, image), the same cut in all four
// full-size kernels.  A workgroup is 256/G pixel slots of G lanes; the G lanes of a slot own the channels of one pixel, K elements
// (float4 when C % 4 == 0 and the pointers are 16-byte aligned, else float) per lane, and the channel sums of a pixel are an xor
// butterfly inside those G lanes.  Reductions over pixels are per-lane serial sums, then a serial sum over the slots through LDS,
// then a serial sum over the chunk partials in the gate kernels, and sums over the batch are serial too: no atomics, so two runs
// give the same bits.  Partials live in the caller's workspace; nothing allocates or synchronises.
#include "scse.h"

namespace vp {
namespace {

// workspace layout, in floats
struct ScseWs {
  size_t pdc, pdws, pdbs, dz2, dz1, dwsi, dbsi, dpool, total;
};
inline ScseWs scse_ws(int B, int C, int Cr, int nchunk) {
  ScseWs w;
  const size_t part = (size_t)B * nchunk * C;
  w.pdc = 0;                                    // forward: channel sums of x per chunk; backward: sum_p dy x per chunk
  w.pdws = part;                                // sum_p ds x per chunk
  w.pdbs = 2 * part;                            // sum_p ds per chunk
  w.dz2 = w.pdbs + (((size_t)B * nchunk + 3) & ~(size_t)3);
  w.dpool = w.dz2 + (size_t)B * C;
  w.dwsi = w.dpool + (size_t)B * C;
  w.dz1 = w.dwsi + (size_t)B * C;
  w.dbsi = w.dz1 + (size_t)B * Cr;
  w.total = w.dbsi + B;
  return w;
}

// ---- forward 1: per-chunk channel sums of x ----------------------------------------------------------------------------------------
template <typename T, int G, int K>
__global__ void __launch_bounds__(256) scse_pool_kernel(const float* __restrict__ x, float* __restrict__ part, int HW, int C, int ppc) {
  constexpr int S = 256 / G, W = sizeof(T) / 4;
  __shared__ T sh[S][G * K];
  const int b = blockIdx.y, chunk = blockIdx.x, j = threadIdx.x % G, slot = threadIdx.x / G, nel = C / W;
  const int p0 = chunk * ppc, p1 = min(HW, p0 + ppc);
  const T* xb = reinterpret_cast<const T*>(x + (size_t)b * HW * C);
  T acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) zero(acc[k]);
#pragma unroll 4
  for (int p = p0 + slot; p < p1; p += S) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = j + k * G;
      if (e < nel) acc[k] = add(acc[k], xb[(size_t)p * nel + e]);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) sh[slot][k * G + j] = acc[k];
  __syncthreads();
  if (slot == 0) {
    T* out = reinterpret_cast<T*>(part + ((size_t)b * gridDim.x + chunk) * C);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = j + k * G;
      if (e >= nel) continue;
      T t = sh[0][k * G + j];
      for (int s = 1; s < S; ++s) t = add(t, sh[s][k * G + j]);
      out[e] = t;
    }
  }
}

// ---- forward 2: channel gate, one workgroup per image ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) scse_gate_fwd_kernel(const float* __restrict__ part, const float* __restrict__ w1,
                                                            const float* __restrict__ b1, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, float* __restrict__ pool,
                                                            float* __restrict__ hid, float* __restrict__ cgate, int HW, int C, int Cr,
                                                            int nchunk) {
  __shared__ float sp[kScseMaxC], shid[kScseMaxC];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inv = 1.f / (float)HW;
  for (int c = tid; c < C; c += 256) {
    const float* pp = part + (size_t)b * nchunk * C + c;
    float a = 0.f;
#pragma unroll 8
    for (int k = 0; k < nchunk; ++k) a += pp[(size_t)k * C];
    a *= inv;
    sp[c] = a;
    pool[(size_t)b * C + c] = a;
  }
  __syncthreads();
  for (int h = wave; h < Cr; h += 4) {
    float a = 0.f;
    for (int c = lane; c < C; c += 64) a += w1[(size_t)h * C + c] * sp[c];
    a = fmaxf(wave_sum(a) + b1[h], 0.f);
    if (lane == 0) {
      shid[h] = a;
      hid[(size_t)b * Cr + h] = a;
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float a = b2[c];
    for (int h = 0; h < Cr; ++h) a += w2[(size_t)c * Cr + h] * shid[h];
    cgate[(size_t)b * C + c] = sigmoidf(a);
  }
}

// ---- forward 3: spatial gate and y = x (c + s) [+ ReLU] ------------------------------------------------------------------------------
template <typename T, int G, int K>
__global__ void __launch_bounds__(256) scse_apply_kernel(const float* __restrict__ x, const float* __restrict__ cgate,
                                                         const float* __restrict__ wsw, const float* __restrict__ bs,
                                                         float* __restrict__ y, float* __restrict__ sgate, int HW, int C, int ppc,
                                                         int do_relu) {
  constexpr int S = 256 / G, W = sizeof(T) / 4, U = 2;
  const int b = blockIdx.y, j = threadIdx.x % G, slot = threadIdx.x / G, nel = C / W;
  const int p0 = blockIdx.x * ppc, p1 = min(HW, p0 + ppc);
  const T* xb = reinterpret_cast<const T*>(x + (size_t)b * HW * C);
  T* yb = reinterpret_cast<T*>(y + (size_t)b * HW * C);
  const T* cgb = reinterpret_cast<const T*>(cgate + (size_t)b * C);
  const T* wv = reinterpret_cast<const T*>(wsw);
  T cg[K], w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = j + k * G;
    zero(cg[k]);
    zero(w[k]);
    if (e < nel) {
      cg[k] = cgb[e];
      w[k] = wv[e];
    }
  }
  const float bsv = bs[0];
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
      const int p = q + u * S + slot;
      const float s = sigmoidf(slot_sum<G>(d[u]) + bsv);
      if (p >= p1) continue;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int e = j + k * G;
        if (e >= nel) continue;
        T o = mul(v[u][k], adds(cg[k], s));
        if (do_relu) o = relu(o);
        yb[(size_t)p * nel + e] = o;
      }
      if (j == 0) sgate[(size_t)b * HW + p] = s;
    }
  }
}

// ---- backward 1: dx without the pooling term (skipped when dx is null), and the per-chunk partials of dc, dw_s, db_s ----------------------------------------
template <typename T, int G, int K>
__global__ void __launch_bounds__(256) scse_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                       const float* __restrict__ cgate, const float* __restrict__ wsw,
                                                       const float* __restrict__ sgate, float* __restrict__ dx,
                                                       float* __restrict__ pdc, float* __restrict__ pdws, float* __restrict__ pdbs,
                                                       int HW, int C, int ppc, int do_relu) {
  constexpr int S = 256 / G, W = sizeof(T) / 4, U = 2;
  __shared__ T sh_dc[S][G * K], sh_dw[S][G * K];
  __shared__ float sh_db[S];
  const int b = blockIdx.y, chunk = blockIdx.x, j = threadIdx.x % G, slot = threadIdx.x / G, nel = C / W;
  const int p0 = chunk * ppc, p1 = min(HW, p0 + ppc);
  const size_t img = (size_t)b * HW * C;
  const T* xb = reinterpret_cast<const T*>(x + img);
  const T* gb = reinterpret_cast<const T*>(dy + img);
  T* dxb = dx ? reinterpret_cast<T*>(dx + img) : nullptr;
  const T* cgb = reinterpret_cast<const T*>(cgate + (size_t)b * C);
  const T* wv = reinterpret_cast<const T*>(wsw);
  T cg[K], w[K], a_dc[K], a_dw[K];
  float a_db = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = j + k * G;
    zero(cg[k]);
    zero(w[k]);
    zero(a_dc[k]);
    zero(a_dw[k]);
    if (e < nel) {
      cg[k] = cgb[e];
      w[k] = wv[e];
    }
  }
  for (int q = p0; q < p1; q += S * U) {
    T v[U][K], g[U][K];
    float t[U], sv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = q + u * S + slot;
      t[u] = 0.f;
      sv[u] = p < p1 ? sgate[(size_t)b * HW + p] : 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int e = j + k * G;
        zero(v[u][k]);
        zero(g[u][k]);
        if (p < p1 && e < nel) {
          v[u][k] = xb[(size_t)p * nel + e];
          g[u][k] = gb[(size_t)p * nel + e];
        }
        if (do_relu) g[u][k] = mask_pos(g[u][k], v[u][k]);
        t[u] += dot(g[u][k], v[u][k]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = q + u * S + slot;
      const float s = sv[u];
      const float ds = slot_sum<G>(t[u]) * s * (1.f - s);      // 0 for a pixel past the chunk: its x and dy were read as 0
      a_db += ds;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int e = j + k * G;
        a_dc[k] = add(a_dc[k], mul(g[u][k], v[u][k]));
        a_dw[k] = add(a_dw[k], muls(v[u][k], ds));
        if (dxb && p < p1 && e < nel) dxb[(size_t)p * nel + e] = add(mul(g[u][k], adds(cg[k], s)), muls(w[k], ds));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    sh_dc[slot][k * G + j] = a_dc[k];
    sh_dw[slot][k * G + j] = a_dw[k];
  }
  if (j == 0) sh_db[slot] = a_db;
  __syncthreads();
  const size_t row = (size_t)b * gridDim.x + chunk;
  if (slot == 0) {
    T* odc = reinterpret_cast<T*>(pdc + row * C);
    T* odw = reinterpret_cast<T*>(pdws + row * C);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = j + k * G;
      if (e >= nel) continue;
      T a = sh_dc[0][k * G + j], d = sh_dw[0][k * G + j];
      for (int s = 1; s < S; ++s) {
        a = add(a, sh_dc[s][k * G + j]);
        d = add(d, sh_dw[s][k * G + j]);
      }
      odc[e] = a;
      odw[e] = d;
    }
  }
  if (threadIdx.x == 0) {
    float a = sh_db[0];
    for (int s = 1; s < S; ++s) a += sh_db[s];
    pdbs[row] = a;
  }
}

// ---- backward 2: per image, finish dc / dw_s / db_s over the chunks and push dc through the two small layers ---------------------
__global__ void __launch_bounds__(256) scse_gate_bwd_kernel(const float* __restrict__ pdc, const float* __restrict__ pdws,
                                                            const float* __restrict__ pdbs, const float* __restrict__ w1,
                                                            const float* __restrict__ w2, const float* __restrict__ hid,
                                                            const float* __restrict__ cgate, float* __restrict__ dz2,
                                                            float* __restrict__ dz1, float* __restrict__ dwsi,
                                                            float* __restrict__ dbsi, float* __restrict__ dpool, int HW, int C, int Cr,
                                                            int nchunk) {
  __shared__ float s2[kScseMaxC], s1[kScseMaxC];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = tid; c < C; c += 256) {
    const float* pa = pdc + (size_t)b * nchunk * C + c;
    const float* pw = pdws + (size_t)b * nchunk * C + c;
    float a = 0.f, d = 0.f;
#pragma unroll 8
    for (int k = 0; k < nchunk; ++k) {
      a += pa[(size_t)k * C];
      d += pw[(size_t)k * C];
    }
    const float cg = cgate[(size_t)b * C + c];
    a *= cg * (1.f - cg);
    s2[c] = a;
    dz2[(size_t)b * C + c] = a;
    dwsi[(size_t)b * C + c] = d;
  }
  if (wave == 3) {                       // nchunk <= 256: four strided terms per lane, then the butterfly
    float a = 0.f;
    for (int k = lane; k < nchunk; k += 64) a += pdbs[(size_t)b * nchunk + k];
    a = wave_sum(a);
    if (lane == 0) dbsi[b] = a;
  }
  __syncthreads();
  for (int h = wave; h < Cr; h += 4) {
    float a = 0.f;
    for (int c = lane; c < C; c += 64) a += w2[(size_t)c * Cr + h] * s2[c];
    a = wave_sum(a);
    a = hid[(size_t)b * Cr + h] > 0.f ? a : 0.f;
    if (lane == 0) {
      s1[h] = a;
      dz1[(size_t)b * Cr + h] = a;
    }
  }
  __syncthreads();
  const float inv = 1.f / (float)HW;
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    for (int h = 0; h < Cr; ++h) a += w1[(size_t)h * C + c] * s1[h];
    dpool[(size_t)b * C + c] = a * inv;
  }
}

// ---- backward 3: parameter gradients, each one serial sum over the batch ---------------------------------------------------------------
__global__ void __launch_bounds__(256) scse_param_grads_kernel(const float* __restrict__ dz2, const float* __restrict__ dz1,
                                                               const float* __restrict__ dwsi, const float* __restrict__ dbsi,
                                                               const float* __restrict__ pool, const float* __restrict__ hid,
                                                               float* __restrict__ dw1, float* __restrict__ db1,
                                                               float* __restrict__ dw2, float* __restrict__ db2,
                                                               float* __restrict__ dws, float* __restrict__ dbs, int B, int C, int Cr) {
  const int n1 = Cr * C, total = 2 * n1 + 2 * C + Cr + 1;
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float a = 0.f;
  if (i < n1) {                                   // dW1[h][c] = sum_b dz1[b][h] pool[b][c]
    const int h = i / C, c = i % C;
    for (int b = 0; b < B; ++b) a += dz1[(size_t)b * Cr + h] * pool[(size_t)b * C + c];
    dw1[i] = a;
    return;
  }
  i -= n1;
  if (i < n1) {                                   // dW2[c][h] = sum_b dz2[b][c] hid[b][h]
    const int c = i / Cr, h = i % Cr;
    for (int b = 0; b < B; ++b) a += dz2[(size_t)b * C + c] * hid[(size_t)b * Cr + h];
    dw2[i] = a;
    return;
  }
  i -= n1;
  if (i < C) {
    for (int b = 0; b < B; ++b) a += dz2[(size_t)b * C + i];
    db2[i] = a;
    return;
  }
  i -= C;
  if (i < C) {
    for (int b = 0; b < B; ++b) a += dwsi[(size_t)b * C + i];
    dws[i] = a;
    return;
  }
  i -= C;
  if (i < Cr) {
    for (int b = 0; b < B; ++b) a += dz1[(size_t)b * Cr + i];
    db1[i] = a;
    return;
  }
  for (int b = 0; b < B; ++b) a += dbsi[b];
  dbs[0] = a;
}

// ---- backward 4: dx += dpool / HW (the mean's gradient, known only after the whole image has been seen) --------------------------
template <typename T, int G, int K>
__global__ void __launch_bounds__(256) scse_dx_pool_kernel(float* __restrict__ dx, const float* __restrict__ dpool, int HW, int C, int ppc) {
  constexpr int S = 256 / G, W = sizeof(T) / 4;
  const int b = blockIdx.y, j = threadIdx.x % G, slot = threadIdx.x / G, nel = C / W;
  const int p0 = blockIdx.x * ppc, p1 = min(HW, p0 + ppc);
  T* dxb = reinterpret_cast<T*>(dx + (size_t)b * HW * C);
  const T* dpb = reinterpret_cast<const T*>(dpool + (size_t)b * C);
  T dp[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    zero(dp[k]);
    if (j + k * G < nel) dp[k] = dpb[j + k * G];
  }
#pragma unroll 4
  for (int p = p0 + slot; p < p1; p += S) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = j + k * G;
      if (e < nel) dxb[(size_t)p * nel + e] = add(dxb[(size_t)p * nel + e], dp[k]);
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" size_t vp_scse_workspace_bytes(int B, int HW, int C, int hidden) {
  if (B <= 0 || HW <= 0 || C <= 0 || hidden <= 0 || hidden > C) return 0;
  const ScsePlan pl = scse_plan(B, HW, C);
  return scse_ws(B, C, hidden, pl.nchunk).total * sizeof(float);
}

extern "C" int vp_scse_fwd_f32(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* w_s,
                               const float* b_s, float* y, float* pool, float* hid, float* cgate, float* sgate, int B, int HW, int C,
                               int hidden, int relu, void* ws, size_t ws_bytes, vp_stream stream) {
  if (int rc = scse_check_dims("vp_scse_fwd_f32", B, HW, C, hidden)) return rc;      // first: an empty hidden layer has null weights
  VP_REQUIRE(x && w1 && b1 && w2 && b2 && w_s && b_s && y && pool && hid && cgate && sgate && ws, "vp_scse_fwd_f32: null pointer");
  const int Cr = hidden;
  const ScsePlan pl = scse_plan(B, HW, C);
  const ScseWs lay = scse_ws(B, C, Cr, pl.nchunk);
  if (ws_bytes < lay.total * sizeof(float))
    return fail(VP_ERR_WORKSPACE, "vp_scse_fwd_f32: workspace of %zu bytes, %zu needed", ws_bytes, lay.total * sizeof(float));
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws + lay.pdc;
  const dim3 grid(pl.nchunk, B), blk(256);
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(cgate) && aligned16(w_s) && aligned16(ws);
  if (int rc = scse_check_path("vp_scse_fwd_f32", vec, C)) return rc;
#define SCSE_POOL(T, G, K) hipLaunchKernelGGL((scse_pool_kernel<T, G, K>), grid, blk, 0, s, x, part, HW, C, pl.ppc)
  if (vec) SCSE_DISPATCH(float4, C / 4, SCSE_POOL);
  else SCSE_DISPATCH(float, C, SCSE_POOL);
#undef SCSE_POOL
  hipLaunchKernelGGL(scse_gate_fwd_kernel, dim3(B), blk, 0, s, (const float*)part, w1, b1, w2, b2, pool, hid, cgate, HW, C, Cr, pl.nchunk);
#define SCSE_APPLY(T, G, K) \
  hipLaunchKernelGGL((scse_apply_kernel<T, G, K>), grid, blk, 0, s, x, (const float*)cgate, w_s, b_s, y, sgate, HW, C, pl.ppc, relu)
  if (vec) SCSE_DISPATCH(float4, C / 4, SCSE_APPLY);
  else SCSE_DISPATCH(float, C, SCSE_APPLY);
#undef SCSE_APPLY
  return check_launch("vp_scse_fwd_f32");
}

extern "C" int vp_scse_bwd_f32(const float* x, const float* dy, const float* w1, const float* w2, const float* w_s, const float* pool,
                               const float* hid, const float* cgate, const float* sgate, float* dx, float* dw1, float* db1, float* dw2,
                               float* db2, float* dw_s, float* db_s, int B, int HW, int C, int hidden, int relu, void* ws,
                               size_t ws_bytes, vp_stream stream) {
  if (int rc = scse_check_dims("vp_scse_bwd_f32", B, HW, C, hidden)) return rc;
  VP_REQUIRE(x && dy && w1 && w2 && w_s && pool && hid && cgate && sgate && dw1 && db1 && dw2 && db2 && dw_s && db_s && ws,
             "vp_scse_bwd_f32: null pointer");
  const int Cr = hidden;
  const ScsePlan pl = scse_plan(B, HW, C);
  const ScseWs lay = scse_ws(B, C, Cr, pl.nchunk);
  if (ws_bytes < lay.total * sizeof(float))
    return fail(VP_ERR_WORKSPACE, "vp_scse_bwd_f32: workspace of %zu bytes, %zu needed", ws_bytes, lay.total * sizeof(float));
  hipStream_t s = (hipStream_t)stream;
  float* f = (float*)ws;
  const dim3 grid(pl.nchunk, B), blk(256);
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(dy) && aligned16(dx) && aligned16(cgate) && aligned16(w_s) && aligned16(ws);
  if (int rc = scse_check_path("vp_scse_bwd_f32", vec, C)) return rc;
#define SCSE_BWD(T, G, K)                                                                                                             \
  hipLaunchKernelGGL((scse_bwd_kernel<T, G, K>), grid, blk, 0, s, x, dy, cgate, w_s, sgate, dx, f + lay.pdc, f + lay.pdws, f + lay.pdbs, \
                     HW, C, pl.ppc, relu)
  if (vec) SCSE_DISPATCH(float4, C / 4, SCSE_BWD);
  else SCSE_DISPATCH(float, C, SCSE_BWD);
#undef SCSE_BWD
  hipLaunchKernelGGL(scse_gate_bwd_kernel, dim3(B), blk, 0, s, (const float*)(f + lay.pdc), (const float*)(f + lay.pdws),
                     (const float*)(f + lay.pdbs), w1, w2, hid, cgate, f + lay.dz2, f + lay.dz1, f + lay.dwsi, f + lay.dbsi, f + lay.dpool,
                     HW, C, Cr, pl.nchunk);
  const int total = 2 * Cr * C + 2 * C + Cr + 1;
  hipLaunchKernelGGL(scse_param_grads_kernel, dim3((total + 255) / 256), blk, 0, s, (const float*)(f + lay.dz2), (const float*)(f + lay.dz1),
                     (const float*)(f + lay.dwsi), (const float*)(f + lay.dbsi), pool, hid, dw1, db1, dw2, db2, dw_s, db_s, B, C, Cr);
#define SCSE_DXP(T, G, K) \
  hipLaunchKernelGGL((scse_dx_pool_kernel<T, G, K>), grid, blk, 0, s, dx, (const float*)(f + lay.dpool), HW, C, pl.ppc)
  if (!dx) {      // the caller wants the parameter gradients alone: no dx store above, no pooling term here
  } else if (vec) SCSE_DISPATCH(float4, C / 4, SCSE_DXP);
  else SCSE_DISPATCH(float, C, SCSE_DXP);
#undef SCSE_DXP
  return check_launch("vp_scse_bwd_f32");
}
