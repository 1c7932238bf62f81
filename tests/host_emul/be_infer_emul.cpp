// Host emulation of csrc/be_infer.hip: the SAME tile bodies (csrc/be_infer.h), compiled for the host, run over every tile of every
// image and head with a plain float array standing for LDS.  A phase loop walks all 256 "threads" where the kernel runs one each,
// and tile_sync() is nothing.  The array is refilled with NaN before every tile, so a read of LDS the tile did not write shows.
#include <cmath>
#include <vector>

#include "../../vae_play_amd/csrc/be_infer.h"

using namespace vp::be;

namespace {

template <int CMID>
int up_run(const float* x, size_t xhs, const float* params, float* y, int heads, int B, int H, int W, int cin) {
  const UpLds L = up_lds(cin, CMID);
  std::vector<float> lds(L.total);
  std::vector<float> acc((size_t)NT * CMID);
  const int th = (H + TH - 1) / TH, tw = (W + TW - 1) / TW;
  for (int head = 0; head < heads; ++head)
    for (int b = 0; b < B; ++b)
      for (int t = 0; t < th * tw; ++t) {
        std::fill(lds.begin(), lds.end(), NAN);
        up_tile<CMID, 1>(lds.data(), x + head * xhs + (size_t)b * H * W * cin, params + (size_t)head * up_params(cin, CMID).total,
                         y + ((size_t)head * B + b) * 4 * H * W * CMID, H, W, cin, (t / tw) * TH, (t % tw) * TW, 0,
                         reinterpret_cast<float(*)[CMID]>(acc.data()));
      }
  return 0;
}

template <int C>
int pred_run(const float* x, size_t xhs, const float* params, float* logits, unsigned char* mask, float threshold, int heads, int B, int H,
             int W) {
  std::vector<float> lds(pred_lds(C).total);
  const int th = (H + TH - 1) / TH, tw = (W + TW - 1) / TW;
  for (int head = 0; head < heads; ++head)
    for (int b = 0; b < B; ++b)
      for (int t = 0; t < th * tw; ++t) {
        std::fill(lds.begin(), lds.end(), NAN);
        const size_t img = ((size_t)head * B + b) * H * W;
        pred_tile<C, 1>(lds.data(), x + head * xhs + (size_t)b * H * W * C, params + (size_t)head * pred_params(C).total, logits + img,
                        mask ? mask + img : nullptr, threshold, H, W, (t / tw) * TH, (t % tw) * TW, 0);
      }
  return 0;
}

}  // namespace

extern "C" {

int emul_be_tile_h() { return TH; }
int emul_be_tile_w() { return TW; }
int emul_be_supported(int cin, int cmid) { return up_supported(cin, cmid) ? 1 : 0; }
int emul_be_up_params_floats(int cin, int cmid) { return up_supported(cin, cmid) ? up_params(cin, cmid).total : 0; }
int emul_be_pred_params_floats(int c) { return pred_supported(c) ? pred_params(c).total : 0; }
int emul_be_up_lds_floats(int cin, int cmid) { return up_lds(cin, cmid).total; }
int emul_be_pred_lds_floats(int c) { return pred_lds(c).total; }

int emul_be_up_pack(const float* w1, const float* g1, const float* b1, const float* m1, const float* v1, const float* w2, const float* g2,
                    const float* b2, const float* m2, const float* v2, float eps, float* params, int cin, int cmid) {
  if (!up_supported(cin, cmid)) return -1;
  for (int i = 0; i < up_params(cin, cmid).total; ++i)
    params[i] = up_pack_elem(i, w1, BnRef{g1, b1, m1, v1}, w2, BnRef{g2, b2, m2, v2}, (double)eps, cin, cmid);
  return 0;
}

int emul_be_pred_pack(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, float* params,
                      int c) {
  if (!pred_supported(c)) return -1;
  for (int i = 0; i < pred_params(c).total; ++i) params[i] = pred_pack_elem(i, w1, b1, w2, b2, w3, b3, c);
  return 0;
}

int emul_be_up(const float* x, size_t xhs, const float* params, float* y, int heads, int B, int H, int W, int cin, int cmid) {
  if (!up_supported(cin, cmid)) return -1;
  switch (cmid) {
    case 2: return up_run<2>(x, xhs, params, y, heads, B, H, W, cin);
    case 4: return up_run<4>(x, xhs, params, y, heads, B, H, W, cin);
    case 8: return up_run<8>(x, xhs, params, y, heads, B, H, W, cin);
    default: return up_run<16>(x, xhs, params, y, heads, B, H, W, cin);
  }
}

int emul_be_pred(const float* x, size_t xhs, const float* params, float* logits, unsigned char* mask, float threshold, int heads, int B,
                 int H, int W, int c) {
  switch (c) {
    case 2: return pred_run<2>(x, xhs, params, logits, mask, threshold, heads, B, H, W);
    case 4: return pred_run<4>(x, xhs, params, logits, mask, threshold, heads, B, H, W);
    case 8: return pred_run<8>(x, xhs, params, logits, mask, threshold, heads, B, H, W);
    default: return -1;
  }
}

}  // extern "C"
