// Segmentation evaluation: per image and per head the loss terms of train_BE.py:58-59, the confusion counts at the
// deployment threshold and a tolerant boundary match, read from the logit planes where a plan left them.  The reference has no
// counterpart (it writes PNG overlays); the loss arithmetic is be_loss_partial_kernel's (elementwise.hip).
//
// A workgroup owns one tile of SE_TH rows x SE_TW columns of one plane; (tile, image, head) is the grid.  A lane takes four
// consecutive pixels of a row per item -- one 16-byte load of the logits and one of the targets when rows are 16-byte aligned (VEC),
// four bounds-checked scalar loads each otherwise -- and SE_U items are loaded before the first is used.  Lane sums are fp32 (at most
// 64 pixels), then fp64 through the wave tree and LDS to ONE partial per workgroup; a second launch adds each image's partials in a
// fixed order.  No atomics: two runs give the same bits.
//
// tol > 0 (TOL): the workgroup also walks the tol halo rows above and below its tile (clipped at the image) and packs the bits
// P = (x >= threshold), T = (t >= target_threshold) into LDS words, 32 columns a word, with one more word on each side for the four
// columns next to the tile (absent at the image's border, so zero).  A pixel of P is matched when a bit of T lies in its
// (2 tol + 1)^2 window: the rows of the window are ORed first, the row of three words is then ORed with its own shifts, the count is
// a popcount.  Rows and words outside the image are never written and stay zero, so the window clips at all four borders, and a
// tile never sees another image or head.  tol == 0 instantiates none of this.
#include <cfloat>
#include "common.h"

namespace vp {
namespace {

constexpr int SE_NT = 256;                       // threads per workgroup
constexpr int SE_TH = 32;                        // tile rows
constexpr int SE_TW = 512;                       // tile columns: 16 words of 32 bits
constexpr int SE_MAXTOL = 4;
constexpr int SE_U = 4;                          // items (16-byte load pairs) in flight per lane
constexpr int SE_WORDS = SE_TW / 32 + 2;         // + the left and the right halo word
constexpr int SE_LROWS = SE_TH + 2 * SE_MAXTOL;

struct SegPartial {                              // one workgroup's result: 64 bytes
  double s[4];                                   // sum bce, sum p t, sum p, sum t
  int c[6];                                      // |P|, |T|, |P & T|, matched_pred, matched_target, nonfinite
  int pad[2];
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// four pixels of a row from column col on, those at or past column `end` as 0.0f; returns how many are inside (0..4).
// VEC: rows are 16-byte aligned and col, end are multiples of 4, so the four are inside together.
template <bool VEC>
__device__ __forceinline__ int load4(const float* __restrict__ row, int col, int end, float (&v)[4]) {
  const int n = max(0, min(4, end - col));
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if constexpr (VEC) {
    if (n > 0) {
      const float4 q = *reinterpret_cast<const float4*>(row + col);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) v[j] = row[col + j];
  }
  return n;
}

__device__ __forceinline__ unsigned bits_ge(const float (&v)[4], float thr, int n) {
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) m |= (unsigned)(j < n && v[j] >= thr) << j;       // a NaN compares false
  return m;
}

template <bool TOL, bool VEC>
__global__ void __launch_bounds__(SE_NT) seg_eval_tile_kernel(const float* __restrict__ logits, size_t logit_head_stride,
                                                              const float* __restrict__ targets, size_t target_head_stride,
                                                              SegPartial* __restrict__ part, int H, int W, int ntx, float thr,
                                                              float tthr, int tol) {
  __shared__ unsigned Pb[TOL ? SE_LROWS : 1][SE_WORDS], Tb[TOL ? SE_LROWS : 1][SE_WORDS];
  __shared__ double shs[4][4];
  __shared__ int shc[6][4];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const size_t image = (size_t)blockIdx.y * H * W;
  const float* __restrict__ x = logits + blockIdx.z * logit_head_stride + image;
  const float* __restrict__ t = targets + blockIdx.z * target_head_stride + image;
  const int r0 = ty * SE_TH, r1 = min(H, r0 + SE_TH);            // the tile's rows and columns, half-open
  const int c0 = tx * SE_TW, c1 = min(W, c0 + SE_TW);
  const int rlo = TOL ? max(0, r0 - tol) : r0, rhi = TOL ? min(H, r1 + tol) : r1;      // with the halo rows
  const int gpr = (((c1 - c0 + 3) >> 2) + 7) & ~7;               // items per row: a multiple of 8, so eight lanes in a row make a word
  const int nitems = (rhi - rlo) * gpr;

  if constexpr (TOL) {
    for (int i = tid; i < SE_LROWS * SE_WORDS; i += SE_NT) {
      (&Pb[0][0])[i] = 0u;
      (&Tb[0][0])[i] = 0u;
    }
    __syncthreads();
  }

  float s[4] = {0.f, 0.f, 0.f, 0.f};
  int c[6] = {0, 0, 0, 0, 0, 0};
  for (int base = 0; base < nitems; base += SE_NT * SE_U) {      // (every lane walks every round: the word shuffles need them all)
    float xv[SE_U][4], tv[SE_U][4];
    int nv[SE_U], row[SE_U], g[SE_U];
#pragma unroll
    for (int u = 0; u < SE_U; ++u) {
      const int i = base + u * SE_NT + tid;
      const bool live = i < nitems;
      const int rr = live ? i / gpr : 0;
      g[u] = live ? i - rr * gpr : 0;
      row[u] = rlo + rr;
      const int col = c0 + 4 * g[u];
      nv[u] = load4<VEC>(x + row[u] * W, col, live ? c1 : 0, xv[u]);
      load4<VEC>(t + row[u] * W, col, live ? c1 : 0, tv[u]);
    }
#pragma unroll
    for (int u = 0; u < SE_U; ++u) {
      const unsigned pn = bits_ge(xv[u], thr, nv[u]), tn = bits_ge(tv[u], tthr, nv[u]);
      if (!TOL || (row[u] >= r0 && row[u] < r1)) {               // a pixel of the tile itself: the sums and the plain counts
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float xj = xv[u][j], tj = tv[u][j];
          const bool in = j < nv[u];
          const float e = __expf(-fabsf(xj));
          float p, q;
          sigmoid_pair(xj, e, p, q);
          s[0] += in ? fmaxf(xj, 0.f) - xj * tj + log1pf(e) : 0.f;
          s[1] += in ? p * tj : 0.f;
          s[2] += in ? p : 0.f;
          s[3] += tj;                                            // (0.0f outside)
          c[5] += in && !(fabsf(xj) <= FLT_MAX);
        }
        c[0] += __popc(pn);
        c[1] += __popc(tn);
        c[2] += __popc(pn & tn);
      }
      if constexpr (TOL) {
        const int sh = (g[u] & 7) * 4;                           // gpr % 8 == 0 and SE_NT % 8 == 0: g & 7 == lane & 7
        unsigned pw = pn << sh, tw = tn << sh;
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
          pw |= __shfl_xor(pw, off, 64);
          tw |= __shfl_xor(tw, off, 64);
        }
        if ((tid & 7) == 0 && base + u * SE_NT + tid < nitems) {
          const int lr = row[u] - r0 + SE_MAXTOL, w = 1 + (g[u] >> 3);
          Pb[lr][w] = pw;
          Tb[lr][w] = tw;
        }
      }
    }
  }

  if constexpr (TOL) {
    // the four columns left and right of the tile, where the image goes on
    for (int i = tid; i < (rhi - rlo) * 2; i += SE_NT) {
      const int rw = rlo + (i >> 1), right = i & 1;
      if (right ? c0 + SE_TW < W : c0 > 0) {
        const int col = right ? c0 + SE_TW : c0 - 4;
        float xh[4], th[4];
        const int n = load4<VEC>(x + rw * W, col, W, xh);
        load4<VEC>(t + rw * W, col, W, th);
        const unsigned pn = bits_ge(xh, thr, n), tn = bits_ge(th, tthr, n);
        const int lr = rw - r0 + SE_MAXTOL;
        Pb[lr][right ? SE_WORDS - 1 : 0] = right ? pn : pn << 28;
        Tb[lr][right ? SE_WORDS - 1 : 0] = right ? tn : tn << 28;
      }
    }
    __syncthreads();
    const int nw = (c1 - c0 + 31) >> 5;
    for (int i = tid; i < (r1 - r0) * (SE_TW / 32); i += SE_NT) {
      const int lr = (i >> 4) + SE_MAXTOL, w = (i & 15) + 1;
      if (w > nw) continue;
      unsigned pl = 0, pc = 0, pr = 0, tl = 0, tc = 0, tr = 0;   // the window's rows ORed: left, centre and right word
      for (int dy = -tol; dy <= tol; ++dy) {
        pl |= Pb[lr + dy][w - 1]; pc |= Pb[lr + dy][w]; pr |= Pb[lr + dy][w + 1];
        tl |= Tb[lr + dy][w - 1]; tc |= Tb[lr + dy][w]; tr |= Tb[lr + dy][w + 1];
      }
      unsigned pd = pc, td = tc;                                 // ... and their columns
      for (int d = 1; d <= tol; ++d) {
        pd |= (pc >> d) | (pr << (32 - d)) | (pc << d) | (pl >> (32 - d));
        td |= (tc >> d) | (tr << (32 - d)) | (tc << d) | (tl >> (32 - d));
      }
      c[3] += __popc(Pb[lr][w] & td);
      c[4] += __popc(Tb[lr][w] & pd);
    }
  }

  const int wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = wave_sum((double)s[k]);
    if ((tid & 63) == 0) shs[k][wave] = v;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int v = wave_sum_i(c[k]);
    if ((tid & 63) == 0) shc[k][wave] = v;
  }
  __syncthreads();
  if (tid == 0) {
    SegPartial out;
    for (int k = 0; k < 4; ++k) out.s[k] = (shs[k][0] + shs[k][1]) + (shs[k][2] + shs[k][3]);
    for (int k = 0; k < 6; ++k) out.c[k] = (shc[k][0] + shc[k][1]) + (shc[k][2] + shc[k][3]);
    out.pad[0] = out.pad[1] = 0;
    part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = out;
  }
}

// one wave per (head, image): lane l adds tiles l, l + 64, ... in order, then the wave tree -- one fixed order
__global__ void __launch_bounds__(64) seg_eval_final_kernel(const SegPartial* __restrict__ part, float* __restrict__ sums,
                                                            float* __restrict__ terms, int* __restrict__ counts, int ntiles, int npix,
                                                            float bce_weight, float smooth, int tol) {
  const size_t img = blockIdx.x;
  const SegPartial* p = part + img * ntiles;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int c[6] = {0, 0, 0, 0, 0, 0};
  for (int k = threadIdx.x; k < ntiles; k += 64) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += p[k].s[j];
#pragma unroll
    for (int j = 0; j < 6; ++j) c[j] += p[k].c[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = wave_sum(s[j]);
#pragma unroll
  for (int j = 0; j < 6; ++j) c[j] = wave_sum_i(c[j]);
  if (threadIdx.x == 0) {
    if (tol == 0) c[3] = c[4] = c[2];
    const double bce = s[0] / (double)npix, dice = (2.0 * s[1] + smooth) / (s[2] + s[3] + smooth);
    for (int j = 0; j < 4; ++j) sums[img * 4 + j] = (float)s[j];
    terms[img * 3 + 0] = (float)bce;
    terms[img * 3 + 1] = (float)dice;
    terms[img * 3 + 2] = (float)(bce_weight * bce + 1.0 - dice);
    for (int j = 0; j < 6; ++j) counts[img * 6 + j] = c[j];
  }
}

inline bool seg_shape_ok(int heads, int B, int H, int W, int tol) {
  return heads > 0 && heads <= 65535 && B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= (1LL << 24) && tol >= 0 &&
         tol <= SE_MAXTOL;
}
inline int seg_tiles_x(int W) { return (W + SE_TW - 1) / SE_TW; }
inline int seg_tiles(int H, int W) { return ((H + SE_TH - 1) / SE_TH) * seg_tiles_x(W); }

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" {

size_t vp_seg_eval_workspace_bytes(int heads, int B, int H, int W, int tol) {
  if (!seg_shape_ok(heads, B, H, W, tol)) return 0;
  return (size_t)heads * B * seg_tiles(H, W) * sizeof(SegPartial);
}

int vp_seg_eval_f32(const float* logits, size_t logit_head_stride, const float* targets, size_t target_head_stride, float* sums,
                    float* terms, int* counts, int heads, int B, int H, int W, float threshold, float target_threshold,
                    float bce_weight, float smooth, int tol, void* ws, size_t ws_bytes, vp_stream stream) {
  const char* what = "vp_seg_eval_f32";
  VP_REQUIRE(logits && targets && sums && terms && counts && ws, "%s: null pointer", what);
  VP_REQUIRE(tol >= 0 && tol <= SE_MAXTOL, "%s: tol must be 0..%d, got %d", what, SE_MAXTOL, tol);
  VP_REQUIRE(seg_shape_ok(heads, B, H, W, tol), "%s: heads, B 1..65535, H, W >= 1 with H * W <= 2^24", what);
  VP_REQUIRE(threshold - threshold == 0.f && target_threshold - target_threshold == 0.f, "%s: the thresholds must be finite", what);
  VP_REQUIRE((((uintptr_t)logits | (uintptr_t)targets) & 3) == 0 && ((uintptr_t)ws & 7) == 0,
             "%s: the planes must be 4-byte aligned, the workspace 8-byte aligned", what);
  const size_t planes = (size_t)B * H * W;
  VP_REQUIRE(heads == 1 || (logit_head_stride >= planes && target_head_stride >= planes), "%s: a head stride is shorter than B * H * W",
             what);
  const int ntx = seg_tiles_x(W), ntiles = seg_tiles(H, W);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = W % 4 == 0 && aligned16(logits, targets) && logit_head_stride % 4 == 0 && target_head_stride % 4 == 0;
  auto* part = static_cast<SegPartial*>(ws);
  const dim3 grid(ntiles, B, heads);
  auto tile = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(SE_NT), 0, s, logits, logit_head_stride, targets, target_head_stride, part, H, W, ntx, threshold,
                       target_threshold, tol);
  };
  return two_stage(
      what, ws_bytes >= vp_seg_eval_workspace_bytes(heads, B, H, W, tol), "workspace too small",
      [&] {
        if (tol > 0) vec ? tile(seg_eval_tile_kernel<true, true>) : tile(seg_eval_tile_kernel<true, false>);
        else vec ? tile(seg_eval_tile_kernel<false, true>) : tile(seg_eval_tile_kernel<false, false>);
      },
      [&] {
        hipLaunchKernelGGL(seg_eval_final_kernel, dim3(heads * B), dim3(64), 0, s, part, sums, terms, counts, ntiles, H * W, bce_weight, smooth,
                           tol);
      });
}

}  // extern "C"
