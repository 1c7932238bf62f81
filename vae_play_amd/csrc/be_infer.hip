// Fused eval-mode inference of the mask / edge heads of models/networks_BE.py:39-66 (MaskNet / EdgeNet: two ``Up`` blocks with
// coordinate channels, three bias-only 3x3 convolutions), exact fp32 on the vector ALUs like small3.hip -- 1 to 66 channels are too
// few for an MFMA tile.  One launch per Up block and one for the predictor, each for all heads (the head index is grid.z); only a
// stage's input and output touch HBM.  The tile bodies are in be_infer.h; DESIGN.md 9.1.
#include "common.h"
#include "be_infer.h"

namespace vp {

using namespace be;

template <int CMID>
__global__ void __launch_bounds__(NT) be_up_kernel(const float* __restrict__ x, size_t x_head_stride, const float* __restrict__ params,
                                                   float* __restrict__ y, int B, int H, int W, int cin, int tiles_w) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.y, head = blockIdx.z;
  const int h0 = (blockIdx.x / tiles_w) * TH, w0 = (blockIdx.x % tiles_w) * TW;
  float acc[1][CMID];
  up_tile<CMID, NT>(lds, x + head * x_head_stride + (size_t)b * H * W * cin, params + (size_t)head * up_params(cin, CMID).total,
                    y + ((size_t)head * B + b) * 4 * H * W * CMID, H, W, cin, h0, w0, threadIdx.x, acc);
}

template <int C>
__global__ void __launch_bounds__(NT) be_pred_kernel(const float* __restrict__ x, size_t x_head_stride, const float* __restrict__ params,
                                                     float* __restrict__ logits, unsigned char* __restrict__ mask, float threshold, int B,
                                                     int H, int W, int tiles_w) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.y, head = blockIdx.z;
  const int h0 = (blockIdx.x / tiles_w) * TH, w0 = (blockIdx.x % tiles_w) * TW;
  const size_t img = ((size_t)head * B + b) * H * W;
  pred_tile<C, NT>(lds, x + head * x_head_stride + (size_t)b * H * W * C, params + (size_t)head * pred_params(C).total, logits + img,
                   mask ? mask + img : nullptr, threshold, H, W, h0, w0, threadIdx.x);
}

__global__ void be_up_pack_kernel(const float* __restrict__ w1, BnRef bn1, const float* __restrict__ w2, BnRef bn2, float eps,
                                  float* __restrict__ params, int cin, int cmid, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) params[i] = up_pack_elem(i, w1, bn1, w2, bn2, (double)eps, cin, cmid);
}

__global__ void be_pred_pack_kernel(const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                    const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3,
                                    float* __restrict__ params, int c, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) params[i] = pred_pack_elem(i, w1, b1, w2, b2, w3, b3, c);
}

// w_out[n][j] = w[n][j] s[n], shift[n] = beta[n] - mean[n] s[n] with s = gamma / sqrt(var + eps): formed in fp64, rounded once
__global__ void be_fold_conv_kernel(const float* __restrict__ w, BnRef bn, float eps, float* __restrict__ w_out, float* __restrict__ shift,
                                    int cout, int cols) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)cout * cols) return;
  const int n = (int)(i / cols);
  w_out[i] = (float)((double)w[i] * bn_scale(bn, n, (double)eps));
  if (i == (size_t)n * cols) shift[n] = bn_shift(bn, n, (double)eps);
}

static bool grid_ok(int heads, int B, int H, int W) { return heads > 0 && heads <= 65535 && B > 0 && B <= 65535 && H > 0 && W > 0; }

}  // namespace vp

using namespace vp;

extern "C" {

int vp_be_infer_supported(int cin, int cmid) { return up_supported(cin, cmid) ? 1 : 0; }

size_t vp_be_up_params_floats(int cin, int cmid) { return up_supported(cin, cmid) ? (size_t)up_params(cin, cmid).total : 0; }

size_t vp_be_predictor_params_floats(int c) { return pred_supported(c) ? (size_t)pred_params(c).total : 0; }

int vp_be_up_pack_f32(const float* w1, const float* gamma1, const float* beta1, const float* mean1, const float* var1, const float* w2,
                      const float* gamma2, const float* beta2, const float* mean2, const float* var2, float eps, float* params, int cin,
                      int cmid, vp_stream stream) {
  VP_REQUIRE(w1 && gamma1 && beta1 && mean1 && var1 && w2 && gamma2 && beta2 && mean2 && var2 && params, "vp_be_up_pack_f32: null pointer");
  VP_REQUIRE(up_supported(cin, cmid) && eps >= 0.f, "vp_be_up_pack_f32: (cin, cmid) must be (16,4) (4,2) (32,8) (8,4) (64,16) or (16,8)");
  const int n = up_params(cin, cmid).total;
  hipLaunchKernelGGL(be_up_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w1, BnRef{gamma1, beta1, mean1, var1}, w2,
                     BnRef{gamma2, beta2, mean2, var2}, eps, params, cin, cmid, n);
  return check_launch("vp_be_up_pack_f32");
}

int vp_be_predictor_pack_f32(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                             float* params, int c, vp_stream stream) {
  VP_REQUIRE(w1 && b1 && w2 && b2 && w3 && b3 && params, "vp_be_predictor_pack_f32: null pointer");
  VP_REQUIRE(pred_supported(c), "vp_be_predictor_pack_f32: c must be 2, 4 or 8");
  const int n = pred_params(c).total;
  hipLaunchKernelGGL(be_pred_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w1, b1, w2, b2, w3, b3, params, c, n);
  return check_launch("vp_be_predictor_pack_f32");
}

int vp_be_fold_conv_f32(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, float* w_out,
                        float* shift, int cout, int cols, vp_stream stream) {
  VP_REQUIRE(w && gamma && beta && mean && var && w_out && shift, "vp_be_fold_conv_f32: null pointer");
  VP_REQUIRE(cout > 0 && cols > 0 && eps >= 0.f, "vp_be_fold_conv_f32: bad sizes");
  const size_t n = (size_t)cout * cols;
  hipLaunchKernelGGL(be_fold_conv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                     BnRef{gamma, beta, mean, var}, eps, w_out, shift, cout, cols);
  return check_launch("vp_be_fold_conv_f32");
}

int vp_be_up_infer_f32(const float* x, size_t x_head_stride, const float* params, float* y, int heads, int B, int H, int W, int cin, int cmid,
                       vp_stream stream) {
  VP_REQUIRE(x && params && y, "vp_be_up_infer_f32: null pointer");
  VP_REQUIRE(up_supported(cin, cmid), "vp_be_up_infer_f32: (cin, cmid) must be (16,4) (4,2) (32,8) (8,4) (64,16) or (16,8)");
  VP_REQUIRE(grid_ok(heads, B, H, W), "vp_be_up_infer_f32: sizes must be positive (heads, B <= 65535)");
  VP_REQUIRE(aligned16(x, params, y) && x_head_stride % 4 == 0, "vp_be_up_infer_f32: operands must be 16-byte aligned");
  const int th = (H + TH - 1) / TH, tw = (W + TW - 1) / TW;
  VP_REQUIRE((long long)th * tw <= 0x7fffffffLL, "vp_be_up_infer_f32: too many tiles");
  const dim3 grid(th * tw, B, heads);
  const size_t lds = (size_t)up_lds(cin, cmid).total * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
#define VP_BE_UP(CM) hipLaunchKernelGGL(be_up_kernel<CM>, grid, dim3(NT), lds, s, x, x_head_stride, params, y, B, H, W, cin, tw)
  switch (cmid) {
    case 2: VP_BE_UP(2); break;
    case 4: VP_BE_UP(4); break;
    case 8: VP_BE_UP(8); break;
    default: VP_BE_UP(16); break;
  }
#undef VP_BE_UP
  return check_launch("vp_be_up_infer_f32");
}

int vp_be_predictor_infer_f32(const float* x, size_t x_head_stride, const float* params, float* logits, unsigned char* mask, float threshold,
                              int heads, int B, int H, int W, int c, vp_stream stream) {
  VP_REQUIRE(x && params && logits, "vp_be_predictor_infer_f32: null pointer");
  VP_REQUIRE(pred_supported(c), "vp_be_predictor_infer_f32: c must be 2, 4 or 8");
  VP_REQUIRE(grid_ok(heads, B, H, W), "vp_be_predictor_infer_f32: sizes must be positive (heads, B <= 65535)");
  VP_REQUIRE(aligned16(x, params) && x_head_stride % 4 == 0, "vp_be_predictor_infer_f32: operands must be 16-byte aligned");
  const int th = (H + TH - 1) / TH, tw = (W + TW - 1) / TW;
  VP_REQUIRE((long long)th * tw <= 0x7fffffffLL, "vp_be_predictor_infer_f32: too many tiles");
  const dim3 grid(th * tw, B, heads);
  const size_t lds = (size_t)pred_lds(c).total * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
#define VP_BE_PRED(CC) hipLaunchKernelGGL(be_pred_kernel<CC>, grid, dim3(NT), lds, s, x, x_head_stride, params, logits, mask, threshold, B, H, W, tw)
  switch (c) {
    case 2: VP_BE_PRED(2); break;
    case 4: VP_BE_PRED(4); break;
    default: VP_BE_PRED(8); break;
  }
#undef VP_BE_PRED
  return check_launch("vp_be_predictor_infer_f32");
}

}  // extern "C"
