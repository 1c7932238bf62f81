/* vaeplay_hip.h -- C ABI of libvaeplay_hip.so, the MI355X (gfx950) back end of the
 * convolutional-VAE training step of kungyao/vae-play.
 *
 * The reference has no FFI of its own (pure PyTorch): the boundary it exposes is
 * nn.Module.forward / loss / optimizer.step.  Every entry point below replaces the ATen/cuDNN
 * call that a reference line dispatches; the citation after each prototype names that line
 * (paths relative to the reference checkout).  The host binds them with ctypes
 * (vae_play_amd/_lib.py); INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers owned by the caller
 *     (PyTorch's allocator); the library never allocates or frees device memory and keeps no
 *     pointer after return;
 *   - activations are NHWC fp32 (= torch channels_last), weights are passed in the reference's
 *     own layouts unless a prototype says "packed";
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); no internal sync;
 *   - return 0 on success, a negative vp_status otherwise; vp_last_error() gives the message
 *     for the calling thread; nothing throws across the ABI;
 *   - `ws`/`ws_bytes`: caller-provided scratch, size from the matching *_workspace_bytes().
 */
#ifndef VAEPLAY_HIP_H
#define VAEPLAY_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vp_stream; /* hipStream_t */

enum vp_status { VP_OK = 0, VP_ERR_ARG = -1, VP_ERR_LAUNCH = -2, VP_ERR_WORKSPACE = -3, VP_ERR_STATE = -4 };
enum vp_act { VP_ACT_NONE = 0, VP_ACT_RELU = 1, VP_ACT_LRELU = 2, VP_ACT_TANH = 3, VP_ACT_SIGMOID = 4 };

int vp_abi_version(void);
const char* vp_last_error(void);

/* ---- layout ------------------------------------------------------------------------------ */
/* NCHW <-> NHWC copies (module I/O is NCHW like the reference's tensors, datasets/dataset.py:68) */
int vp_nchw_to_nhwc_f32(const float* in, float* out, int B, int C, int H, int W, vp_stream stream);
int vp_nhwc_to_nchw_f32(const float* in, float* out, int B, int C, int H, int W, vp_stream stream);

/* 5x5 weight repack.  w_ref is the reference tensor W[Csmall][Cbig][5][5]
 * (nn.Conv2d weight (Cout,Cin,5,5) models/networks.py:14; nn.ConvTranspose2d weight
 * (Cin,Cout,5,5) models/networks.py:38).  p0 = [Csmall][25][Cbig], p1 = [Cbig][25][Csmall];
 * either output may be NULL. */
int vp_pack_w5_f32(const float* w_ref, float* p0, float* p1, int Csmall, int Cbig, vp_stream stream);

/* ---- 5x5 pad-2 convolution families (stride 1 or 2; big = stride * small) ------------------ */
/* small[B,Hs,Ws,Cs] = act(bias + conv5(big[B,s*Hs,s*Ws,Cb]))
 *   replaces nn.Conv2d fwd models/networks.py:27 (EncoderBlock), :100-103 (final conv + Sigmoid,
 *   act = VP_ACT_SIGMOID) and nn.ConvTranspose2d's input gradient (autograd of :43). */
int vp_conv5_gather_f32(const float* big, const float* w_p0, const float* bias, float* small_out,
                        int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int act, vp_stream stream);
/* big[B,s*Hs,s*Ws,Cb] = convT5(small)  (sub-pixel phases, no zero insertion)
 *   replaces nn.ConvTranspose2d fwd models/networks.py:43 (DecoderBlock) and nn.Conv2d's input
 *   gradient (autograd of :27, :100). */
int vp_conv5_scatter_f32(const float* small, const float* w_p1, float* big_out,
                         int B, int Hs, int Ws, int Csmall, int Cbig, int stride, vp_stream stream);
/* dW[Cs][Cb][5][5] (reference layout) = sum_pixels small (x) shifted big
 *   replaces the weight gradient of both layer kinds (autograd of models/networks.py:27,:43,:100). */
size_t vp_conv5_wgrad_workspace_bytes(int B, int Hs, int Ws, int Cbig, int Csmall, int stride);
int vp_conv5_wgrad_f32(const float* big, const float* small, float* dw_ref,
                       int B, int Hs, int Ws, int Cbig, int Csmall, int stride,
                       void* ws, size_t ws_bytes, vp_stream stream);
/* As vp_conv5_wgrad_f32 with a bound on the CUs the launch occupies (see vp_conv5_wgrad_bf16x3_cus; max_cus <= 0: the whole chip;
 * max_cus > 256, more than the chip has, behaves as 256).  Same workspace query as vp_conv5_wgrad_f32. */
int vp_conv5_wgrad_f32_cus(const float* big, const float* small, float* dw_ref, int B, int Hs, int Ws, int Cbig, int Csmall,
                           int stride, int max_cus, void* ws, size_t ws_bytes, vp_stream stream);
/* Exact-fp32 convolution + the statistics pass of the BatchNorm that follows it (models/networks.py:14-16,38-40) in one call, as
 * vp_conv5_*_stats_bf16x3: {pivot, sum(x - pivot), sum((x - pivot)^2)} per (workgroup, channel) from the fp32 accumulators, one
 * finaliser launch for mean / rstd / running statistics (momentum semantics of torch).  vp_conv5_stats_f32_workspace_bytes() == 0:
 * the shape cannot emit them (it splits K, or does not take the fast fp32 path) -- use vp_conv5_*_f32 + vp_bn_stats_f32. */
size_t vp_conv5_stats_f32_workspace_bytes(int family, int B, int Hs, int Ws, int Cbig, int Csmall, int stride);
int vp_conv5_gather_stats_f32(const float* big, const float* w_p0, float* small_out, int B, int Hs, int Ws, int Cbig, int Csmall, int stride,
                              float eps, float momentum, float* mean, float* rstd, float* running_mean, float* running_var, void* ws,
                              size_t ws_bytes, vp_stream stream);
int vp_conv5_scatter_stats_f32(const float* small, const float* w_p1, float* big_out, int B, int Hs, int Ws, int Csmall, int Cbig, int stride,
                               float eps, float momentum, float* mean, float* rstd, float* running_mean, float* running_var, void* ws,
                               size_t ws_bytes, vp_stream stream);

/* ---- k x k generalisation (ks = 1, 3, 4 or 5, padding (ks-1)/2, stride 1 or 2) ----------------------------------
 * The conv/norm/act vocabulary of models/blocks.py:5-34 (nn.Conv2d(k, stride, padding=(k-1)//2)); same three families.
 * ks = 4 (padding 1) is the Style-GAN generator's kernel: myConv2d(.., 4, 2) and nn.ConvTranspose2d(in, out, 4, 2, 1),
 * models/network_Style_GAN.py:49,95-98,116.
 * The big side is passed explicitly (Hb, Wb) so odd sizes work: Hs = floor((Hb + 2*pad - ks)/stride) + 1.
 * Weights: reference tensor W[Csmall][Cbig][ks][ks]; packed p0 = [Csmall][ks*ks][Cbig], p1 = [Cbig][ks*ks][Csmall].
 * The gather family's epilogue: act(acc + bias[n]) with act none | sigmoid | relu (relu: a convolution whose eval-mode BatchNorm
 * is folded into weight and bias, vp_be_fold_conv_f32). */
int vp_pack_w_f32(const float* w_ref, float* p0, float* p1, int Csmall, int Cbig, int ks, vp_stream stream);
int vp_conv_gather_f32(const float* big, const float* w_p0, const float* bias, float* small_out,
                       int B, int Hs, int Ws, int Hb, int Wb, int Cbig, int Csmall, int ks, int stride, int act, vp_stream stream);
int vp_conv_scatter_f32(const float* small, const float* w_p1, float* big_out,
                        int B, int Hs, int Ws, int Hb, int Wb, int Csmall, int Cbig, int ks, int stride, vp_stream stream);
/* vp_conv_scatter_f32 + bias[Cbig] added once to every output pixel (a pixel that no tap reaches holds exactly the bias): the
 * forward pass of nn.ConvTranspose2d(in, out, 4, 2, 1) with its default bias, models/network_Style_GAN.py:49,116, without a
 * second pass over the full-size output.  Always the generic-geometry kernel; bias == NULL is vp_conv_scatter_f32, bit for bit. */
int vp_conv_scatter_bias_f32(const float* small, const float* w_p1, const float* bias, float* big_out,
                             int B, int Hs, int Ws, int Hb, int Wb, int Csmall, int Cbig, int ks, int stride, vp_stream stream);
size_t vp_conv_wgrad_workspace_bytes(int B, int Hs, int Ws, int Hb, int Wb, int Cbig, int Csmall, int ks, int stride);
int vp_conv_wgrad_f32(const float* big, const float* small, float* dw_ref,
                      int B, int Hs, int Ws, int Hb, int Wb, int Cbig, int Csmall, int ks, int stride,
                      void* ws, size_t ws_bytes, vp_stream stream);

/* k x k (k = 1, 3, 4, 5; padding (k-1)/2; explicit big size Hb x Wb as for vp_conv_gather_f32) forms of the three split-bf16
 * families, for the models/blocks.py vocabulary; weights packed by vp_pack_w_split: p0 = [Csmall][k*k][Cbig],
 * p1 = [Cbig][k*k][Csmall], both as bf16 hi/lo planes. */
int vp_pack_w_split(const float* w_ref, void* p0_split, void* p1_split, int Csmall, int Cbig, int ks, vp_stream stream);
int vp_conv_gather_bf16x3(const void* big_split, const void* w_p0_split, const float* bias, float* small_out, int B, int Hs, int Ws,
                          int Hb, int Wb, int Cbig, int Csmall, int ks, int stride, int act, vp_stream stream);
int vp_conv_scatter_bf16x3(const void* small_split, const void* w_p1_split, float* big_out, int B, int Hs, int Ws, int Hb, int Wb,
                           int Csmall, int Cbig, int ks, int stride, vp_stream stream);
/* as vp_conv_scatter_bias_f32 on split planes (models/network_Style_GAN.py:49,116); bias == NULL is vp_conv_scatter_bf16x3 */
int vp_conv_scatter_bias_bf16x3(const void* small_split, const void* w_p1_split, const float* bias, float* big_out, int B, int Hs, int Ws,
                                int Hb, int Wb, int Csmall, int Cbig, int ks, int stride, vp_stream stream);
size_t vp_conv_wgrad_bf16x3_workspace_bytes(int B, int Hs, int Ws, int Hb, int Wb, int Cbig, int Csmall, int ks, int stride);
int vp_conv_wgrad_bf16x3(const void* big_split, const void* small_split, float* dw_ref, int B, int Hs, int Ws, int Hb, int Wb, int Cbig,
                         int Csmall, int ks, int stride, void* ws, size_t ws_bytes, vp_stream stream);
/* ---- split-bf16 ("bf16x3") variants of the three families ------------------------------------------
 * A "split" tensor stores an fp32 tensor of n elements as two bf16 planes in one buffer of 2*n
 * uint16: hi = bf16(x) at [0,n), lo = bf16(x - hi) at [n,2n).  The contraction issues three
 * v_mfma_f32_32x32x16_bf16 per fragment pair (lo*hi + hi*lo + hi*hi) with fp32 accumulation:
 * ~5e-6 relative error per contraction.  Channel counts on the contracted/vector side must be
 * multiples of 8; outputs are plain fp32.  Same reference lines as the f32 entry points above. */
int vp_split_f32(const float* x, void* out_split, size_t n, vp_stream stream);
/* the same for an NHWC tensor [npix][C] whose channel count is not a multiple of 8: planes [npix][Cpad], channels C..Cpad-1
 * zero (models/blocks.py:97-146 AddCoords makes 32 + 2 channels; the heads of models/networks_BE.py:39-89 end in 1 channel) */
int vp_split_pad_f32(const float* x, void* out_split, size_t npix, int C, int Cpad, vp_stream stream);
int vp_pack_w5_split(const float* w_ref, void* p0_split, void* p1_split, int Csmall, int Cbig, vp_stream stream);
int vp_conv5_gather_bf16x3(const void* big_split, const void* w_p0_split, const float* bias, float* small_out,
                           int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int act, vp_stream stream);
int vp_conv5_scatter_bf16x3(const void* small_split, const void* w_p1_split, float* big_out,
                            int B, int Hs, int Ws, int Csmall, int Cbig, int stride, vp_stream stream);
/* Final conv + bias + sigmoid (nn.Conv2d(64, C, k5, s1, p2) + nn.Sigmoid, models/networks.py:100-103, C = 1 or 3) in split-bf16
 * arithmetic on the matrix cores: the 25 taps x C outputs are the MFMA column dimension ("tap-in-N", csrc/narrow.hip); fp32 NHWC
 * input (split into bf16 hi/lo in registers) and the fp32 packed weights P0 [C][25][64] of vp_pack_w5_f32, fp32 output. */
int vp_conv5_smallout_bf16x3(const float* big, const float* w_p0, const float* bias, float* small_out, int B, int H, int W,
                             int Cbig, int Csmall, int act, vp_stream stream);
/* ... and its weight gradient dW[C][64][5][5] = sum_pixels dlogit x shifted activation, with the 25 taps x C gradient channels as
 * the MFMA row dimension ("taps in M", csrc/edge.hip): fp32 activation [B,H,W,64] and fp32 dlogit [B,H,W,C] in, reference weight
 * layout out; deterministic slab reduction.  The workspace query returns 0 for shapes it does not take (width not a multiple of
 * 64, height not of 16): use vp_conv5_wgrad_f32 there. */
size_t vp_conv5_smallout_wgrad_bf16x3_workspace_bytes(int B, int H, int W, int Cbig, int Csmall);
int vp_conv5_smallout_wgrad_bf16x3(const float* big, const float* small, float* dw_ref, int B, int H, int W, int Cbig, int Csmall,
                                   void* ws, size_t ws_bytes, vp_stream stream);
/* The same weight gradient in exact fp32 (v_mfma_f32_32x32x2_f32, the dlogit patch and u as fp32 in LDS, the pixels of a super-step
 * split over the four waves and their partial sums added in a fixed order): same workspace size, same slab layout and reduction. */
size_t vp_conv5_smallout_wgrad_f32_workspace_bytes(int B, int H, int W, int Cbig, int Csmall);
int vp_conv5_smallout_wgrad_f32(const float* big, const float* small, float* dw_ref, int B, int H, int W, int Cbig, int Csmall,
                                void* ws, size_t ws_bytes, vp_stream stream);
/* First encoder conv (nn.Conv2d(C, 64, k5, s2, p2, bias=False) with C = 1 or 3 image channels, models/networks.py:14 via :55):
 * its im2col is materialised once per step as split planes [B*Hs*Ws][KC] (KC = vp_im2col5s2_cols(C): 96 / 64), after which the
 * forward convolution is vp_conv_gather_bf16x3(ks = 1, Cbig = KC) and the weight gradient vp_conv_wgrad_bf16x3(ks = 1) on the
 * MFMA kernels; the packed weight / the gradient use the same column order (r*GW + q*C + cin) and are converted from / to the
 * reference layout [64][C][5][5] by the two small kernels below.  x is NCHW (nchw = 1) or NHWC fp32. */
int vp_im2col5s2_cols(int C);
int vp_im2col5s2_split_f32(const float* x, void* out_split, int B, int C, int Hb, int Wb, int nchw, vp_stream stream);
int vp_pack_w_im2col5_split(const float* w_ref, void* out_split, int Cout, int C, vp_stream stream);
int vp_unpack_dw_im2col5_f32(const float* dw_cols, float* dw_ref, int Cout, int C, vp_stream stream);
/* The same im2col and weight re-ordering as plain fp32 ([B*Hs*Ws][KC] and [Cout][KC]) for the exact-f32 plan: the first conv and its
 * weight gradient then run as 1x1 layers through vp_conv_gather_f32 / vp_conv_wgrad_f32 (ks = 1) on the fp32 matrix cores. */
int vp_im2col5s2_f32(const float* x, float* out, int B, int C, int Hb, int Wb, int nchw, vp_stream stream);
int vp_pack_w_im2col5_f32(const float* w_ref, float* out, int Cout, int C, vp_stream stream);
/* Convolution + BatchNorm batch statistics in one call (replaces nn.Conv2d / nn.ConvTranspose2d followed by the statistics
 * pass of nn.BatchNorm2d(momentum=0.9), models/networks.py:14-16,27-28 and :38-40,43-44): the convolution's epilogue emits
 * per-workgroup {pivot, sum(x - pivot), sum((x - pivot)^2)} per output channel from its accumulators and one finaliser
 * launch produces mean / rstd and updates the running buffers exactly as vp_bn_stats_f32 does -- the activation is not read
 * again for its statistics.  family: 0 = gather, 1 = scatter.  vp_conv5_stats_workspace_bytes() == 0 means that this launch
 * shape cannot emit statistics (split-K layers, the narrow-channel halo kernels): use the plain entry point + vp_bn_stats_f32. */
size_t vp_conv5_stats_workspace_bytes(int family, int B, int Hs, int Ws, int Cbig, int Csmall, int stride);
int vp_conv5_gather_stats_bf16x3(const void* big_split, const void* w_p0_split, float* small_out,
                                 int B, int Hs, int Ws, int Cbig, int Csmall, int stride, float eps, float momentum,
                                 float* mean, float* rstd, float* running_mean, float* running_var,
                                 void* ws, size_t ws_bytes, vp_stream stream);
int vp_conv5_scatter_stats_bf16x3(const void* small_split, const void* w_p1_split, float* big_out,
                                  int B, int Hs, int Ws, int Csmall, int Cbig, int stride, float eps, float momentum,
                                  float* mean, float* rstd, float* running_mean, float* running_var,
                                  void* ws, size_t ws_bytes, vp_stream stream);
/* Input gradient of the final conv (nn.Conv2d(64 -> C, k5, s1, p2), models/networks.py:100-103, autograd backward) for C = 1 | 3
 * image channels: big_out[b,h,w,cf] = sum_{r,q,n} small[b, h-r+2, w-q+2, n] * w_ref[n][cf][r][q], fp32 NHWC operands, reference weight
 * layout, split-bf16 arithmetic on the matrix cores with one kernel row of taps (5*C contiguous floats of `small`) per MFMA k-step. */
int vp_conv5_smallin_dgrad_bf16x3(const float* small, const float* w_ref, float* big_out, int B, int H, int W, int Csmall, int Cbig,
                                  vp_stream stream);
/* The same input gradient (models/networks.py:100-103 backward) in exact fp32: v_mfma_f32_32x32x2_f32 on the same rows-in-K tiling. */
int vp_conv5_smallin_dgrad_f32(const float* small, const float* w_ref, float* big_out, int B, int H, int W, int Csmall, int Cbig,
                               vp_stream stream);
/* Forward pass of a stride-1 first conv on a 1- or 3-channel image (nn.Conv2d(C, 32 | 64, k5, s1, p2) + ReLU, the VAE-GAN
 * discriminator's first layer, models/networks.py:160-163): big_out[b,h,w,cf] = act(bias[cf] + sum small[b,h+r-2,w+q-2,n] * w_ref[cf][n][r][q]),
 * fp32 NHWC operands, reference weight layout, act none | relu; the same rows-in-K kernel as vp_conv5_smallin_dgrad_bf16x3. */
int vp_conv5_smallin_fwd_bf16x3(const float* small, const float* w_ref, const float* bias, float* big_out, int B, int H, int W, int Csmall,
                                int Cbig, int act, vp_stream stream);
/* The same layer with the result written as split bf16 planes instead of fp32: out_hi = the hi plane of this launch's first image, the
 * lo plane lies plane_elems elements behind it (plane_elems >= B * H * W * Cbig: several launches may fill consecutive pieces of one
 * split tensor).  The planes equal, bit for bit, vp_split_f32 of what vp_conv5_smallin_fwd_bf16x3 writes; the fp32 tensor -- the
 * discriminator's largest -- is neither written nor read back. */
int vp_conv5_smallin_fwd_planes_bf16x3(const float* small, const float* w_ref, const float* bias, void* out_hi, size_t plane_elems, int B,
                                       int H, int W, int Csmall, int Cbig, int act, vp_stream stream);
size_t vp_conv5_wgrad_bf16x3_workspace_bytes(int B, int Hs, int Ws, int Cbig, int Csmall, int stride);
int vp_conv5_wgrad_bf16x3(const void* big_split, const void* small_split, float* dw_ref,
                          int B, int Hs, int Ws, int Cbig, int Csmall, int stride,
                          void* ws, size_t ws_bytes, vp_stream stream);
/* The same with a bound on the CUs the launch occupies.  The row-of-taps kernel (csrc/wgrad5.h: one kernel row of 5 taps per
 * workgroup, replaces cuDNN's weight gradient behind models/networks.py:14,38) owns a whole CU per work item; a caller that runs the
 * weight gradient BESIDE other kernels -- the fused step's side stream -- leaves the rest of the chip to them (160 of 256 CUs is the
 * measured optimum there).  max_cus <= 0: the whole chip (= vp_conv5_wgrad_bf16x3); max_cus > 256, more than the chip has, behaves
 * as 256.  Same workspace query, same result up to the summation order of the pixel ranges. */
int vp_conv5_wgrad_bf16x3_cus(const void* big_split, const void* small_split, float* dw_ref,
                              int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int max_cus,
                              void* ws, size_t ws_bytes, vp_stream stream);
/* Weight gradient of a 3x3 / stride 1 / padding 1 nn.Conv2d with a handful of channels on both sides (Cin <= 40, Cout <= 8: the mask /
 * edge heads of models/networks_BE.py:39-66 via models/blocks.py:9-17), exact fp32 on the vector ALUs: x (B, H, W, Cin) and dy (B, H, W,
 * Cout) NHWC, dw_ref (Cout, Cin, 3, 3); bit-reproducible.  vp_conv3_small_wgrad_workspace_bytes() == 0: shape not taken. */
size_t vp_conv3_small_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int vp_conv3_small_wgrad_f32(const float* x, const float* dy, float* dw_ref, int B, int H, int W, int Cin, int Cout,
                             void* ws, size_t ws_bytes, vp_stream stream);
/* ... and their forward pass / input gradient: y = bias + conv3x3(x, w) and dx = conv3x3^T(dy, w), one output pixel per thread, exact
 * fp32, reading the reference weight layout (Cout, Cin, 3, 3) directly (no packing, no channel padding). */
int vp_conv3_small_fwd_f32(const float* x, const float* w_ref, const float* bias, float* y, int B, int H, int W, int Cin, int Cout,
                           vp_stream stream);
int vp_conv3_small_dgrad_f32(const float* dy, const float* w_ref, float* dx, int B, int H, int W, int Cin, int Cout, vp_stream stream);
/* Second half of every weight-gradient entry point above (the gradient of nn.Conv2d / nn.ConvTranspose2d weights,
 * models/networks.py:14,38): the K-split launch leaves slab[split][tap][Csmall][Cbig]; this sums the splits in a fixed order
 * (even splits, odd splits, their sum: bit-reproducible, no atomics) and writes the reference layout dw[Csmall][Cbig][tap].
 * variant: -1 = what the library dispatches, 0 = 4-B loads, 1 = 16-B loads (needs Csmall * Cbig % 64 == 0 and 16-B aligned
 * pointers); every variant returns the same bits.  Exposed for callers that split K themselves and for the parity tests. */
int vp_wgrad_slab_reduce_f32(const float* slab, float* dw_ref, int Csmall, int Cbig, int nsplit, int ntaps, int variant,
                             vp_stream stream);
/* producers of split tensors fused into the elementwise passes (y / dx / out may be NULL when only
 * the split copy is wanted) */
/* nn.BatchNorm1d(momentum=0.9) + activation behind nn.Linear (models/networks.py:66-67,89-90), forward and backward, for at most
 * 64 rows (the batch): statistics, finalisation and the normalised output / the two channel sums and the input gradient in ONE
 * launch each, bit-identical to vp_bn_stats_f32 + vp_bn_act_fwd_f32 and to vp_bn_act_bwd_f32 (same arithmetic, step for step). */
int vp_bn_small_fwd_f32(const float* x, int R, int C, float eps, float momentum, const float* gamma, const float* beta, float* mean,
                        float* rstd, float* running_mean, float* running_var, float* y, int act, float slope, vp_stream stream);
int vp_bn_small_bwd_f32(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        float* dx, float* dgamma, float* dbeta, int R, int C, int act, float slope, int batch_stats, vp_stream stream);
int vp_bn_act_fwd_split_f32(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                            float* y, void* y_split, int R, int C, int act, float slope, vp_stream stream);
int vp_bn_act_bwd_split_f32(const float* x, const float* dy, const float* mean, const float* rstd,
                            const float* gamma, const float* beta, float* dx, void* dx_split, float* dgamma, float* dbeta,
                            int R, int C, int act, float slope, int batch_stats,
                            void* ws, size_t ws_bytes, vp_stream stream);
int vp_nchw_to_nhwc_split_f32(const float* in, float* out, void* out_split, int B, int C, int H, int W, vp_stream stream);
/* Every conv weight of a step in ONE launch: job i packs w (reference layout [Csmall][Cbig][5][5]) into p0
 * ([Csmall][25][Cbig]) and/or p1 ([Cbig][25][Csmall_pad]); split = 1 writes bf16 hi/lo planes, 2 fp16 hi/lo planes, 0 fp32.
 * jobs is a HOST array (read during the call only); at most 32 output layouts per batch. */
typedef struct vp_pack_job {
  const float* w;
  void* p0;
  void* p1;
  int Csmall, Cbig, Csmall_pad, split;
} vp_pack_job;
int vp_pack_w5_batch(const vp_pack_job* jobs, int njobs, vp_stream stream);
/* edge layers (1/3 image channels) on the bf16x3 path: the small-channel dimension zero-padded to a multiple of 8.
 * p1_split = [Cbig][25][Csmall_pad] planes; dlogit_split = [npix][Cpad] planes next to the fp32 dlogit [npix][C]. */
int vp_pack_w5_p1_split_padded(const float* w_ref, void* p1_split, int Csmall, int Cbig, int Csmall_pad, vp_stream stream);
int vp_bce_sigmoid_bwd_pad_split_f32(const float* p, const float* t, float gscale, float* dlogit, void* dlogit_split,
                                     size_t npix, int C, int Cpad, vp_stream stream);

/* ---- dense layers ------------------------------------------------------------------------ */
/* C[m][n] = bias[n] + sum_k A(m,k) B(n,k) with element strides (sam,sak) / (sbn,sbk).
 * mode 0: both operands k-contiguous (Linear fwd, models/networks.py:75-77,109)
 * mode 1: A k-contiguous, B n-contiguous (Linear input gradient)
 * mode 2: A m-contiguous, B n-contiguous (Linear weight gradient) */
size_t vp_gemm_workspace_bytes(int M, int N, int K);
int vp_gemm_f32(const float* A, long sam, long sak, const float* B, long sbn, long sbk,
                float* C, int ldc, const float* bias, int M, int N, int K, int mode,
                void* ws, size_t ws_bytes, vp_stream stream);
/* out[c] = sum_r x[r][c]   (bias gradients) */
size_t vp_colsum_workspace_bytes(int R, int C);
int vp_colsum_f32(const float* x, float* out, int R, int C, void* ws, size_t ws_bytes, vp_stream stream);

/* ---- BatchNorm (+ activation) over an [R][C] NHWC view (R = B*H*W, or B for BatchNorm1d) ---- */
/* replaces nn.BatchNorm2d/1d(momentum=0.9) + F.relu  models/networks.py:16,28-29,40,44-45,66-67,89-90;
 * also the norm/act vocabulary of models/blocks.py:19-30. */
size_t vp_bn_workspace_bytes(int R, int C);
/* batch statistics: mean[c], rstd[c] = 1/sqrt(biased_var+eps); if running_* != NULL they are
 * updated in place: run = (1-momentum)*run + momentum*batch (unbiased var), torch semantics. */
int vp_bn_stats_f32(const float* x, int R, int C, float eps, float momentum,
                    float* mean, float* rstd, float* running_mean, float* running_var,
                    void* ws, size_t ws_bytes, vp_stream stream);
/* y = act(gamma*(x-mean)*rstd + beta); gamma/beta may be NULL (affine=False). */
int vp_bn_act_fwd_f32(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                      float* y, int R, int C, int act, float slope, vp_stream stream);
/* backward through act + BN.  batch_stats=1: training-mode formula (statistics depend on x);
 * batch_stats=0: eval mode (mean/rstd constants).  dgamma/dbeta may be NULL.  dx may alias dy. */
int vp_bn_act_bwd_f32(const float* x, const float* dy, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta,
                      int R, int C, int act, float slope, int batch_stats,
                      void* ws, size_t ws_bytes, vp_stream stream);
/* nn.InstanceNorm2d(affine=False, eps) + activation over B images of [R = H*W][C] NHWC (models/blocks.py:22): per-(image,
 * channel) statistics; mean / rstd [B][C] are outputs of the forward and inputs of the backward. */
size_t vp_instnorm_workspace_bytes(int B, int R, int C);
int vp_instnorm_act_fwd_f32(const float* x, float* y, float* mean, float* rstd, int B, int R, int C, float eps, int act,
                            float slope, void* ws, size_t ws_bytes, vp_stream stream);
int vp_instnorm_act_bwd_f32(const float* x, const float* dy, const float* mean, const float* rstd, float* dx, int B, int R, int C,
                            int act, float slope, void* ws, size_t ws_bytes, vp_stream stream);
/* the same with the bf16 hi/lo planes of y / dx written by the apply pass (C % 4 == 0; plane = B * R * C elements): the operand
 * of the split-bf16 convolution that consumes the normalised activation / its input gradient (models/blocks.py:22-30) */
int vp_instnorm_act_fwd_split_f32(const float* x, float* y, void* y_split, float* mean, float* rstd, int B, int R, int C, float eps,
                                  int act, float slope, void* ws, size_t ws_bytes, vp_stream stream);
int vp_instnorm_act_bwd_split_f32(const float* x, const float* dy, const float* mean, const float* rstd, float* dx, void* dx_split, int B,
                                  int R, int C, int act, float slope, void* ws, size_t ws_bytes, vp_stream stream);
/* label-gated pair of convolutions, conv_1(x) * (1 - label) + conv_2(x) * label (models/network_Style_GAN.py:72-79), behind ONE
 * convolution whose weights are the two branches' stacked along the output channel: u is [B][R = H*W][2C] NHWC with branch 1 in
 * channels [0, C) and branch 2 in [C, 2C); label [B] floats; y [B][R][C] = (1 - label[b]) * act(pre_1) + label[b] * act(pre_2).
 * norm = 1: pre_j is InstanceNorm2d(affine=False, eps) of branch j (statistics over the 2C channels; mean / rstd [B][2C] are outputs
 * of the forward and inputs of the backward; needs the workspace).  norm = 0: pre_j = u_j; mean, rstd, ws may be null.
 * y_split / du_split (nullable, C % 4 == 0): bf16 hi/lo planes of y (plane = B*R*C elements) / du (plane = B*R*2C), laid out as by
 * vp_instnorm_act_fwd_split_f32.  The label gets no gradient.  Fixed-order reductions: two runs are bit-identical. */
size_t vp_pair_blend_workspace_bytes(int B, int R, int C);
int vp_pair_blend_fwd_f32(const float* u, const float* label, float* y, void* y_split, float* mean, float* rstd, int B, int R, int C,
                          int norm, float eps, int act, float slope, void* ws, size_t ws_bytes, vp_stream stream);
int vp_pair_blend_bwd_f32(const float* u, const float* dy, const float* label, const float* mean, const float* rstd, float* du,
                          void* du_split, int B, int R, int C, int norm, int act, float slope, void* ws, size_t ws_bytes,
                          vp_stream stream);
/* plain activation (conv + bias + act blocks of models/blocks.py:24-30 with bn=None) */
int vp_act_fwd_f32(const float* x, float* y, size_t n, int act, float slope, vp_stream stream);
/* dx = dy * act'(.) evaluated from the OUTPUT y (relu/lrelu/tanh/sigmoid); dx may alias dy */
int vp_act_bwd_from_y_f32(const float* y, const float* dy, float* dx, size_t n, int act, float slope, vp_stream stream);

/* ---- models/blocks.py helpers (NHWC) ------------------------------------------------------------------------- */
/* F.interpolate(scale_factor=2, mode='bilinear') of blocks.Up (models/blocks.py:145): y[B,2H,2W,C]; and its adjoint */
int vp_upsample2x_bilinear_fwd_f32(const float* x, float* y, int B, int H, int W, int C, vp_stream stream);
int vp_upsample2x_bilinear_bwd_f32(const float* dy, float* dx, int B, int H, int W, int C, vp_stream stream);
/* AddCoords (models/blocks.py:97-112): out[B,H,W,C+2] = cat(x, column index, row index); normalize as if_normalize */
int vp_add_coords_f32(const float* x, float* out, int B, int H, int W, int C, int normalize, vp_stream stream);
/* out[p][0..Cout) = in[p][0..Cout): gradient of AddCoords / channel slice */
int vp_slice_channels_f32(const float* in, float* out, size_t npix, int Cin, int Cout, vp_stream stream);

/* ---- latent: reparameterisation + KL -------------------------------------------------------- */
/* z = eps*exp(0.5*logvar) + mu   (models/networks.py:228-231);
 * kl[b] = -0.5*sum_j(1 + logvar - mu^2 - exp(logvar))  (models/networks.py:270); kl may be NULL */
int vp_latent_fwd_f32(const float* mu, const float* logvar, const float* eps, float* z, float* kl,
                      int B, int Z, vp_stream stream);
/* dmu = dz + gkl[b]*mu ; dlogvar = dz*eps*0.5*exp(0.5*logvar) + gkl[b]*0.5*(exp(logvar)-1)
 * dz may be NULL (KL term only); gkl is per-sample dL/dkl[b] (NULL = 0) */
int vp_latent_bwd_f32(const float* mu, const float* logvar, const float* eps, const float* dz, const float* gkl,
                      float gkl_scalar, float* dmu, float* dlogvar, int B, int Z, vp_stream stream);

/* ---- per-image scoring of a trained VAE (vae_play_amd.infer.FusedVAEInference.score) --------- */
/* The reference has no evaluation loop with a loss; the terms are its KL (models/networks.py:270) and the per-pixel
 * F.binary_cross_entropy(reduction="sum"), kept per image.  Bit-reproducible: fixed-order sums, no atomics. */
/* out[r] = sum_i -[t*max(log p,-100) + (1-t)*max(log(1-p),-100)] over the n elements of row r: p and t dense [rows][n] in the
 * same memory order; the clamp of vp_bce_sum_f32.  ws >= vp_bce_rows_workspace_bytes(rows, n) = rows * ceil(n / 4096) floats. */
size_t vp_bce_rows_workspace_bytes(int rows, int n);
int vp_bce_rows_f32(const float* p, const float* t, int rows, int n, float* out, void* ws, size_t ws_bytes, vp_stream stream);
/* z and kl exactly as vp_latent_fwd_f32 writes them (the same bits; kl may be NULL), and the log density ratio of the draw
 * lr[b] = log p(z_b) - log q(z_b|x_b) = -1/2 sum_j z_j^2 + 1/2 sum_j (eps_j^2 + logvar_j)   (the 2 pi terms cancel) */
int vp_latent_iw_fwd_f32(const float* mu, const float* logvar, const float* eps, float* z, float* kl, float* lr,
                         int B, int Z, vp_stream stream);
/* K-sample importance-weighted bound (Burda et al. 2016; new functionality, no counterpart in the reference).
 * nbce, lr [B][K]: logw[b][k] = -nbce[b][k] + lr[b][k] (logw may be NULL);
 * iwae[b] = max_k logw + log(sum_k exp(logw - max)) - log K; K = 1 returns logw[b][0] exactly */
int vp_iw_bound_f32(const float* nbce, const float* lr, int B, int K, float* logw, float* iwae, vp_stream stream);

/* ---- latent projection through a frozen eval-mode decoder (vae_play_amd.infer.FusedVAEInference.project / decode_grad) ------ */
/* New functionality, no counterpart in the reference.  Bit-reproducible: fixed-order sums, no atomics (csrc/project.hip). */
/* Backward through u = relu(scale*c + shift) (a block with its eval-mode BatchNorm folded) evaluated from the OUTPUT u:
 * dx[r][ch] = (dy[r][ch] * scale[ch]) * (u[r][ch] > 0 ? 1 : 0) over an [R][C] (NHWC) view.  u is given as fp32 (u) or as bf16 split
 * planes (u_split; the mask is hi + lo > 0), exactly one of the two.  dx (fp32) and / or dx_split (the planes vp_split_f32 makes of
 * that fp32 result) are written; dx may alias dy.  16-byte accesses when C % 4 == 0 and the pointers are aligned, else scalar. */
int vp_affine_relu_bwd_f32(const float* dy, const float* u, const void* u_split, const float* scale, float* dx, void* dx_split,
                           size_t R, int C, vp_stream stream);
/* out[r] = sum_i mask * -[t*max(log p,-100) + (1-t)*max(log(1-p),-100)] and dlogit = mask * (p - t) (the convention of
 * vp_bce_sigmoid_bwd_f32) in one read of p, t, mask: dense [rows][n] in one memory order.  mask == NULL: all ones, and out carries
 * the bits vp_bce_rows_f32 returns on the same p and t.  ws >= vp_bce_masked_rows_bwd_workspace_bytes(rows, n). */
size_t vp_bce_masked_rows_bwd_workspace_bytes(int rows, int n);
int vp_bce_masked_rows_bwd_f32(const float* p, const float* t, const float* mask, int rows, int n, float* out, float* dlogit, void* ws,
                               size_t ws_bytes, vp_stream stream);
/* One torch.optim.Adam step (no amsgrad, no weight decay) on z [rows][Z] with moments m, v and gradient g + prior_weight*z.  The
 * step count is READ FROM DEVICE MEMORY: step_count[0] = steps taken so far, this call is step step_count[0] + 1, so that one
 * captured graph serves any number of iterations.  The counter is advanced by a separate one-thread launch that this call enqueues
 * AFTER the update, never by the update itself.  prior (may be NULL): prior[r] = prior_weight/2 * |z_r|^2 of the z that was read.
 * With prior_weight = 0 the update writes the bits vp_adam_f32 writes at the same step with grad_scale = 1 on the same rows * Z
 * elements (below that kernel's streaming-loop threshold of 16.7 M elements).
 * g, m, v and step_count all NULL: no update, prior alone. */
int vp_latent_adam_f32(float* z, const float* g, float* m, float* v, int* step_count, int rows, int Z, float lr, float beta1,
                       float beta2, float eps, float prior_weight, float* prior, vp_stream stream);

/* ---- per-pixel BCE ------------------------------------------------------------------------ */
/* out[0] = sum_i -[t*max(log p,-100) + (1-t)*max(log(1-p),-100)]  (torch F.binary_cross_entropy,
 * reduction='sum'; call form train_BE_font.py:107).  p and t may have different memory order only
 * if the caller made them match. */
size_t vp_reduce_workspace_bytes(size_t n);
int vp_bce_sum_f32(const float* p, const float* t, size_t n, float* out, void* ws, size_t ws_bytes, vp_stream stream);
/* dp = g * (p - t) / max(p*(1-p), 1e-12)   (torch's BCE backward) ; g read from device scalar gptr * gscale */
int vp_bce_bwd_f32(const float* p, const float* t, const float* gptr, float gscale, float* dp, size_t n, vp_stream stream);
/* fused sigmoid+BCE backward on the logits: dlogit = gscale * (p - t) */
int vp_bce_sigmoid_bwd_f32(const float* p, const float* t, float gscale, float* dlogit, size_t n, vp_stream stream);
/* ---- font network pieces (models/networks_BE_font.py, models/blocks.py:66-96, train_BE_font.py:158) ------------- */
/* nn.AdaptiveAvgPool2d((1,1)) on NHWC: out[b][c] = mean_p x[b][p][c]; bwd: dx[b][p][c] = dy[b][c] / HW */
int vp_global_avgpool_fwd_f32(const float* x_nhwc, float* out, int B, int HW, int C, vp_stream stream);
int vp_global_avgpool_bwd_f32(const float* dy, float* dx_nhwc, int B, int HW, int C, vp_stream stream);
/* nn.Softmax(dim=-1) over R rows of n; bwd: dx = y * (dy - sum_j dy_j y_j) */
int vp_softmax_rows_fwd_f32(const float* x, float* y, int R, int n, vp_stream stream);
int vp_softmax_rows_bwd_f32(const float* y, const float* dy, float* dx, int R, int n, vp_stream stream);
/* F.cross_entropy(logits, labels) with torch's defaults (mean over the R rows; labels int64 class indices): train_BE_GAN.py:135,159
 * (d_type_loss / g_type_loss), train_BE_font.py:109.  loss[0] = mean_r (logsumexp(x_r) - x_r[label_r]); prob (R x n) = softmax rows,
 * kept for the backward pass: dlogits = g[0] / R * (prob - onehot(labels)).  Bit-reproducible (fixed-order sum in fp64). */
int vp_cross_entropy_fwd_f32(const float* logits, const long long* labels, float* loss, float* prob, int R, int n, vp_stream stream);
int vp_cross_entropy_bwd_f32(const float* prob, const long long* labels, const float* gptr, float* dlogits, int R, int n, vp_stream stream);
/* F.l1_loss(a, b) (mean): out[0]; ws >= 2 * vp_reduce_workspace_bytes(n).  bwd: da = g * sign(a-b) / n, db = -da */
int vp_l1_mean_f32(const float* a, const float* b, size_t n, float* out, void* ws, size_t ws_bytes, vp_stream stream);
int vp_l1_mean_bwd_f32(const float* a, const float* b, const float* gptr, float* da, float* db, size_t n, vp_stream stream);

/* ---- segmentation loss of train_BE.py:58-59: bce_weight * F.binary_cross_entropy_with_logits(x, t) (mean over B*n)
 * + compute_dice_loss(sigmoid(x), t, smooth) (tools/ops.py:12-19) for B samples of n logits each.
 * fwd: loss[0] and sums[B][4] = {sum bce, sum p*t, sum p, sum t} per sample (kept for the backward);
 * bwd: dlogits = g * d loss / d logits with g read from the device scalar gptr (NULL = 1). */
size_t vp_be_loss_workspace_bytes(int B, int n);
int vp_be_loss_fwd_f32(const float* logits, const float* targets, float* loss, float* sums, int B, int n, float bce_weight,
                       float smooth, void* ws, size_t ws_bytes, vp_stream stream);
int vp_be_loss_bwd_f32(const float* logits, const float* targets, const float* sums, const float* gptr, float* dlogits, int B,
                       int n, float bce_weight, float smooth, vp_stream stream);

/* plain dice loss on probabilities (tools/ops.py:178-185, used by edge_loss :187-215): 1 - mean_b (2 I_b + s)/(P_b + T_b + s);
 * sums[B][4] as above (entry 0 unused); workspace = vp_be_loss_workspace_bytes(B, n). */
int vp_dice_loss_fwd_f32(const float* probs, const float* targets, float* loss, float* sums, int B, int n, float smooth, void* ws,
                         size_t ws_bytes, vp_stream stream);
int vp_dice_loss_bwd_f32(const float* probs, const float* targets, const float* sums, const float* gptr, float* dprobs, int B, int n,
                         float smooth, vp_stream stream);

/* ---- 0.5*(a-b)^2 (VaeGan.loss, models/networks.py:267 "nle" per element, :273 "mse" summed per row) ---- */
int vp_half_sqdiff_f32(const float* a, const float* b, float* out, size_t n, vp_stream stream);
/* out[r] = sum_j 0.5*(a[r][j]-b[r][j])^2 for R contiguous rows of n_per_row elements */
int vp_half_sqdiff_rowsum_f32(const float* a, const float* b, float* out, int R, int n_per_row, vp_stream stream);
/* da = g*(a-b), db = -da (either may be NULL); g has one value per row (g_per_row=1) or per element (0) */
int vp_half_sqdiff_bwd_f32(const float* a, const float* b, const float* g, float* da, float* db, int R, int n_per_row,
                           int g_per_row, vp_stream stream);
/* ---- VAE-GAN loss heads for the fused VAE-GAN step (VaeGan.loss, models/networks.py:275-279; weights of train.py:63-66) ---- */
/* logit [3B] = discriminator scores before F.sigmoid (models/networks.py:190) of (original | reconstructed | sampled);
 * p_out = sigmoid(logit); sums[0..2] = sum_b -log(p + 1e-3) over the originals and sum_b -log(1 - p + 1e-3) over the reconstructed /
 * sampled rows (:275-277); dlogit = coef * d(sums[0] + sums[1] + sums[2]) / dlogit.  Any output may be NULL. */
int vp_gan_head_f32(const float* logit, int B, float coef, float* p_out, float* sums, float* dlogit, vp_stream stream);
/* loss[0] = scale * F.smooth_l1_loss(targets, cat(a, b, dim=1), reduction="sum") (models/networks.py:279, beta = 1) with targets
 * [B][n1 + n2], a [B][n1], b [B][n2] (DirectDecoder's two heads, models/networks.py:144-147); da, db = d loss / d a, b. */
int vp_smooth_l1_cat_f32(const float* targets, const float* a, const float* b, int B, int n1, int n2, float scale, float* loss,
                         float* da, float* db, vp_stream stream);
/* out[0] = sum x */
int vp_sum_f32(const float* x, size_t n, float* out, void* ws, size_t ws_bytes, vp_stream stream);
/* loss tail of the composed VAE step (F.binary_cross_entropy(x_tilde, x, reduction='sum') + the KL of
 * models/networks.py:270 summed over the batch, as train.py:63 does) in two launches: recon = sum of per-pixel BCE,
 * kl_sum = sum_b kl[b], loss = (recon + kl_sum) * loss_scale (device scalars; loss_scale = 1/B gives the per-image loss). */
int vp_vae_loss_f32(const float* x_tilde, const float* x, size_t n, const float* kl, int B, float* recon, float* kl_sum,
                    float* loss, float loss_scale, void* ws, size_t ws_bytes, vp_stream stream);
/* out = a + b (the two latent heads' input gradients, models/networks.py:76-77 backward) */
int vp_add_f32(const float* a, const float* b, float* out, size_t n, vp_stream stream);

/* ---- fp16-pair operands: a cheaper contraction for the same convolutions (nn.Conv2d / nn.ConvTranspose2d of
 * models/networks.py:14,38 and their autograd backward); engine precision "f16x2" --------------------------------------------------
 * Operands are fp16 pairs (x = hi + lo, format 1 below).  `products` = 3: al*bh + ah*bl + ah*bh with v_mfma_f32_32x32x16_f16
 * (up to 22 significant bits per operand, ~1e-6 relative: the forward layers, so OUTPUTS keep the bf16x3 tolerance);
 * `products` = 2: (ah + al)*bh, two MFMAs instead of three -- the operand that keeps only its hi plane (11 significant bits,
 * 2^-12 rms rounding) is the weight in the gather / scatter families and `big` in the weight gradient: DECLARED TOLERANCE ~2e-4
 * relative per layer, used for the backward layers (gradients).  fp16's range is narrow (|x| <= 65504, 2^-24 absolute step below
 * 2^-14), so a producer of GRADIENT planes multiplies by a power of two (`scale`) and the consuming launch multiplies its
 * accumulators by out_scale = 1/scale; activations and weights use scale 1 (values saturate at +-65504 instead of overflowing).
 * `products` = 1 (gather / scatter entry points only; fused inference, precision "f16"): ah*bh, ONE MFMA per fragment pair -- only the hi
 * plane of either operand is fetched (11 significant bits each; the lo planes of the buffers are never read and may be left unwritten).
 * Replaces models/networks.py:14,38 in eval mode, where activations behind a folded BatchNorm + ReLU are O(1); no gradient form.
 * Split formats: 0 = bf16 pair (the *_bf16x3 entry points), 1 = fp16 pair (the *_f16* entry points); same buffer sizes.
 * Every *_fmt producer with format 0 and scale 1 is bit-identical to the entry point without the suffix. */
#define VP_SPLIT_BF16 0
#define VP_SPLIT_F16 1
int vp_split_fmt_f32(const float* x, void* out_split, size_t n, int fmt, float scale, vp_stream stream);
int vp_nchw_to_nhwc_split_fmt_f32(const float* in, float* out, void* out_split, int B, int C, int H, int W, int fmt, vp_stream stream);
int vp_bn_act_fwd_split_fmt_f32(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                float* y, void* y_split, int R, int C, int act, float slope, int fmt, vp_stream stream);
/* dx (fp32, unscaled) and/or dx_split = split(scale * dx) */
int vp_bn_act_bwd_split_fmt_f32(const float* x, const float* dy, const float* mean, const float* rstd,
                                const float* gamma, const float* beta, float* dx, void* dx_split, float* dgamma, float* dbeta,
                                int R, int C, int act, float slope, int batch_stats, int fmt, float scale,
                                void* ws, size_t ws_bytes, vp_stream stream);
/* the same with a sticky saturation flag: *saturated (device int, owned and zeroed by the caller) is set to 1 when fmt = fp16 pairs and
 * |scale * dx| exceeds fp16's range (65504) somewhere -- the planes then hold clamped values; engine.FusedVAEStep(precision="f16x2")
 * reads the flag in sync_counters() and asks for a smaller grad_scale16 */
int vp_bn_act_bwd_split_fmt_sat_f32(const float* x, const float* dy, const float* mean, const float* rstd,
                                    const float* gamma, const float* beta, float* dx, void* dx_split, float* dgamma, float* dbeta,
                                    int R, int C, int act, float slope, int batch_stats, int fmt, float scale, int* saturated,
                                    void* ws, size_t ws_bytes, vp_stream stream);
int vp_im2col5s2_split_fmt_f32(const float* x, void* out_split, int B, int C, int Hb, int Wb, int nchw, int fmt, vp_stream stream);
int vp_pack_w_im2col5_split_fmt(const float* w_ref, void* out_split, int Cout, int C, int fmt, vp_stream stream);
/* the three families; arguments as the *_bf16x3 entry points plus products (1 | 2 | 3) and out_scale (workspace queries of the weight
 * gradient: the *_bf16x3 ones).  The weight gradient exists in the two-product form only; the *_stats_* entry points take
 * products 2 | 3 and return VP_ERR_ARG for 1. */
int vp_conv5_gather_f16(const void* big_split, const void* w_p0_split, const float* bias, float* small_out,
                        int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int act, int products, float out_scale, vp_stream stream);
int vp_conv_gather_f16(const void* big_split, const void* w_p0_split, const float* bias, float* small_out, int B, int Hs, int Ws,
                       int Hb, int Wb, int Cbig, int Csmall, int ks, int stride, int act, int products, float out_scale, vp_stream stream);
int vp_conv5_scatter_f16(const void* small_split, const void* w_p1_split, float* big_out,
                         int B, int Hs, int Ws, int Csmall, int Cbig, int stride, int products, float out_scale, vp_stream stream);
int vp_conv_scatter_f16(const void* small_split, const void* w_p1_split, float* big_out, int B, int Hs, int Ws, int Hb, int Wb,
                        int Csmall, int Cbig, int ks, int stride, int products, float out_scale, vp_stream stream);
int vp_conv5_wgrad_f16x2(const void* big_split, const void* small_split, float* dw_ref, int B, int Hs, int Ws, int Cbig,
                         int Csmall, int stride, float out_scale, void* ws, size_t ws_bytes, vp_stream stream);
int vp_conv5_wgrad_f16x2_cus(const void* big_split, const void* small_split, float* dw_ref, int B, int Hs, int Ws, int Cbig,
                             int Csmall, int stride, float out_scale, int max_cus, void* ws, size_t ws_bytes, vp_stream stream);
int vp_conv_wgrad_f16x2(const void* big_split, const void* small_split, float* dw_ref, int B, int Hs, int Ws, int Hb, int Wb, int Cbig,
                        int Csmall, int ks, int stride, float out_scale, void* ws, size_t ws_bytes, vp_stream stream);
/* forward layers with the BatchNorm statistics in the epilogue (as vp_conv5_*_stats_bf16x3; own workspace query because the
 * launch shapes differ where bf16x3 uses its halo / pipelined kernels) */
size_t vp_conv5_stats_f16_workspace_bytes(int family, int B, int Hs, int Ws, int Cbig, int Csmall, int stride);
int vp_conv5_gather_stats_f16(const void* big_split, const void* w_p0_split, float* small_out,
                              int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int products, float eps, float momentum,
                              float* mean, float* rstd, float* running_mean, float* running_var,
                              void* ws, size_t ws_bytes, vp_stream stream);
int vp_conv5_scatter_stats_f16(const void* small_split, const void* w_p1_split, float* big_out,
                               int B, int Hs, int Ws, int Csmall, int Cbig, int stride, int products, float eps, float momentum,
                               float* mean, float* rstd, float* running_mean, float* running_var,
                               void* ws, size_t ws_bytes, vp_stream stream);


/* ---- inference: eval-mode BatchNorm folded into the convolution's epilogue --------------------------------------------------
 * In eval() a BatchNorm is the per-channel affine map y = s x + t with s = gamma / sqrt(running_var + eps) and
 * t = beta - running_mean s (models/networks.py:16,28-29 and :40,44-45 under the eval() branch of VaeGan.forward,
 * models/networks.py:248-258; the torch.no_grad() reconstruction of train.py:95-96).  vp_bn_fold_f32 writes s, t (and
 * rstd = 1 / sqrt(running_var + eps) for the layers that keep vp_bn_act_fwd_f32) once per set of weights, formed in fp64 and rounded
 * once; gamma / beta may be NULL (affine=False), each output may be NULL. */
int vp_bn_fold_f32(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, float* scale,
                   float* shift, float* rstd, int C, vp_stream stream);
/* nn.Conv2d / nn.ConvTranspose2d (k5, p2, no bias) + eval-mode nn.BatchNorm2d + F.relu of a block in ONE launch (replaces
 * models/networks.py:27-29 and :43-45 in eval mode): v = act(fma(acc, scale[n], shift[n])), act none | relu, written as fp32 NHWC
 * (out_f32) and / or as the split planes of the next layer's operand (out_split, bf16x3 only: hi plane, then lo plane, the layout
 * and rounding of vp_bn_act_fwd_split_f32); at least one output, 16-byte aligned.  The f32 entry points take out_split == NULL only.
 * vp_conv5_affine_supported(family 0 gather | 1 scatter, precision 0 bf16x3 | 1 f32 | 2 one-product f16, ...) == 0: this launch shape does not fuse (its
 * plain launch splits K, or its channel counts are outside the instantiated tiles: contracted side a multiple of 64 [f32: 32],
 * output side >= 64 and a multiple of 8): use the plain entry point + vp_bn_act_fwd_split_f32. */
int vp_conv5_affine_supported(int family, int precision, int B, int Hs, int Ws, int Cbig, int Csmall, int stride);
int vp_conv5_gather_affine_bf16x3(const void* big_split, const void* w_p0_split, const float* scale, const float* shift, float* out_f32,
                                  void* out_split, int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int act, vp_stream stream);
int vp_conv5_scatter_affine_bf16x3(const void* small_split, const void* w_p1_split, const float* scale, const float* shift, float* out_f32,
                                   void* out_split, int B, int Hs, int Ws, int Csmall, int Cbig, int stride, int act, vp_stream stream);
int vp_conv5_gather_affine_f32(const float* big, const float* w_p0, const float* scale, const float* shift, float* out_f32, void* out_split,
                               int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int act, vp_stream stream);
int vp_conv5_scatter_affine_f32(const float* small, const float* w_p1, const float* scale, const float* shift, float* out_f32, void* out_split,
                                int B, int Hs, int Ws, int Csmall, int Cbig, int stride, int act, vp_stream stream);
/* The same block in one-product fp16 (precision code 2 of vp_conv5_affine_supported; the same shape rules as bf16x3): replaces
 * models/networks.py:14,38 with :27-29 / :43-45 in eval mode.  Operands are fp16 planes (format 1) of which only the hi planes are read,
 * contraction as products = 1 above, v = act(fma(acc, scale[n], shift[n])).  out_split is written according to out_fmt:
 *   0  bf16 pair, both planes (exactly the bf16x3 entry point's write: the consumer is a bf16x3 kernel)
 *   1  fp16 pair, both planes (vp_split_fmt_f32's rounding, saturating at +-65504)
 *   2  the fp16 hi plane only; the lo plane of the buffer is NOT written (the consumer is a one-product layer). */
int vp_conv5_gather_affine_f16(const void* big_split, const void* w_p0_split, const float* scale, const float* shift, float* out_f32,
                               void* out_split, int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int act, int out_fmt,
                               vp_stream stream);
int vp_conv5_scatter_affine_f16(const void* small_split, const void* w_p1_split, const float* scale, const float* shift, float* out_f32,
                                void* out_split, int B, int Hs, int Ws, int Csmall, int Cbig, int stride, int act, int out_fmt,
                                vp_stream stream);

/* ---- inference: the VAE-GAN discriminator's tap and head in eval mode, the folded DirectDecoder (csrc/infer_gan.hip) ---------------
 * vp_disc_tap_eval_f32: c [n][64][C] = the fp32 NHWC output of the convolution of conv[recon_level] at 8 x 8 (models/networks.py:
 * 178-183), C a multiple of 32, read once.  act_flat [n][C * 64] = relu(fma(c, scale, shift)) and feat_flat [n][C * 64] = c, both in
 * the reference's NCHW flatten order (what fc.0 reads; the mode "REC" result); with pair_rows = P > 0 (2 P <= n)
 * dist[i] = 1/2 sum (c[i] - c[i + P])^2 for i < P ("mse", :273).  act_flat, feat_flat and (with P = 0) dist may each be NULL.  The sum
 * of a pair has one fixed order that depends on neither n nor the grid: no atomics, bit-reproducible, the same in any batch.
 * vp_disc_head_eval_f32: h [n][H] = fc.0's output; per row logit = sum relu(fma(h, scale, shift)) w + bias[0] (fc.1 in eval mode,
 * fc.3; bias is a device pointer), p = sigmoid(logit) (:198), nl_real = -log(p + 1e-3), nl_fake = -log(1 - p + 1e-3) (:274-276; 1 - p
 * as sigmoid(-logit), without the cancellation).  Each output [n] may be NULL.  Fixed summation order per row.
 * vp_lin_fold_f32: two bias-ed Linear layers without an activation between them as one: w_new [M][K] = w_out [M][N] w [N][K],
 * b_new [M] = w_out b + b_out, M <= 8, fp32 fma over n = 0 .. N - 1 in that order (DirectDecoder, models/networks.py:118-148). */
int vp_disc_tap_eval_f32(const float* c, const float* scale, const float* shift, int n, int C, float* act_flat, float* feat_flat,
                         int pair_rows, float* dist, vp_stream stream);
int vp_disc_head_eval_f32(const float* h, const float* scale, const float* shift, const float* w, const float* bias, int n, int H,
                          float* logit, float* p, float* nl_real, float* nl_fake, vp_stream stream);
int vp_lin_fold_f32(const float* w_out, const float* b_out, const float* w, const float* b, int M, int N, int K, float* w_new,
                    float* b_new, vp_stream stream);

/* ---- inference: the mask / edge heads of models/networks_BE.py:39-66 in eval mode (csrc/be_infer.hip) ---------------
 * MaskNet / EdgeNet = Up(c, c/4, coord) -> Up(c/4, c/8, coord) -> three bias-only 3x3 convolutions, as the reference runs them for
 * inference (test_BE.py:92-98).  Exact fp32, NHWC, `heads` heads per launch: tensors are [heads][B][H][W][C], x_head_stride = floats
 * between two heads' inputs (0: every head reads the same map, as the first Up block does), parameter blocks are packed per head.
 * vp_be_up_infer_f32: one eval-mode Up(cin, cmid, if_add_coord=True) block (models/blocks.py:129-146) in ONE launch: the 3x3
 * convolution cin + 2 -> cmid over x and the two unnormalised coordinate channels (column, row; computed from the pixel position,
 * zero in the padding ring like every other channel), BatchNorm, ReLU, the 3x3 convolution cmid -> cmid, BatchNorm, ReLU, and the 2x
 * bilinear resize (align_corners=False); y [heads][B][2H][2W][cmid].  (cin, cmid) as vp_be_infer_supported() says: (16,4) (4,2) (32,8)
 * (8,4) (64,16) (16,8), the blocks of MaskNet(16 | 32 | 64).
 * vp_be_predictor_infer_f32: the three convolutions c -> 2c -> c -> 1 with their biases and no activation (models/networks_BE.py:48-52)
 * in ONE launch, c = 2 | 4 | 8; logits [heads][B][H][W]; mask (may be NULL) [heads][B][H][W] bytes = logit >= threshold
 * (test_BE.py:35-39 thresholds the raw output).
 * The pack kernels build one head's parameter block (vp_be_*_params_floats() floats; head h's block starts h blocks in) from the
 * reference-layout tensors: the BatchNorms fold as vp_bn_fold_f32 does (fp64, rounded once), the scale INTO the weights, the shift as
 * the sum's first term.  vp_be_fold_conv_f32 does the same for a BatchNorm-ed convolution that runs on the MFMA kernels (aux_convs):
 * w_out [cout][cols] = w s, shift [cout].  16-byte aligned operands. */
int vp_be_infer_supported(int cin, int cmid);
size_t vp_be_up_params_floats(int cin, int cmid);
size_t vp_be_predictor_params_floats(int c);
int vp_be_up_pack_f32(const float* w1, const float* gamma1, const float* beta1, const float* mean1, const float* var1, const float* w2,
                      const float* gamma2, const float* beta2, const float* mean2, const float* var2, float eps, float* params, int cin,
                      int cmid, vp_stream stream);
int vp_be_predictor_pack_f32(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                             float* params, int c, vp_stream stream);
int vp_be_fold_conv_f32(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, float* w_out,
                        float* shift, int cout, int cols, vp_stream stream);
int vp_be_up_infer_f32(const float* x, size_t x_head_stride, const float* params, float* y, int heads, int B, int H, int W, int cin, int cmid,
                       vp_stream stream);
int vp_be_predictor_infer_f32(const float* x, size_t x_head_stride, const float* params, float* logits, unsigned char* mask, float threshold,
                              int heads, int B, int H, int W, int c, vp_stream stream);

/* ---- inference: page compositing for the mask / edge heads (csrc/be_page.hip) ---------------------------------------
 * What the reference's test_BE_manga.py:63-147 (paset_result_on_manga) and :160-225 (paset_edge_result_on_manga) do on the host: the
 * predictions of a page's m bubble crops pasted into one page [H][W][3] uint8 label map, channels (edge, bubble type, content), bit
 * for bit.  Bubble i's logit planes are edges + i * edge_stride and masks + i * mask_stride ([SH][SW] fp32 each, strides in floats;
 * a bit is set unless logit < threshold, so a NaN is set), its page mask page_masks + i * H * W bytes (non-zero = set).
 * desc: m rows of VP_BE_PAGE_DESC_INTS int32 on the device, 16-byte aligned:
 *   0..3   anchor_x, anchor_y, the fp32 bits of (float)SW / (float)size, the fp32 bits of (float)SH / (float)size
 *   4..7   xmin, ymin, xmax, ymax     the bubble's box on the page, half-open
 *   8..11  rx0, ry0, rx1, ry1         kind 1: the content rectangle in crop coordinates, half-open
 *   12..15 label (0..255), kind, 0, 0
 * A page pixel (y, x) inside the box has crop coordinates cy = anchor_y + y - ymin, cx = anchor_x + x - xmin and samples the planes at
 * min((int)floorf(c * scale), S - 1) per axis (torch's nearest resize of the plane to size x size).  kind 0: edge and content bit from
 * edges / masks; kind 1: content = inside the rectangle, edge = inside the rectangle grown by 6 (empty for an empty rectangle);
 * kind 2: content = page mask, edge = OR of the page mask over the 13 x 13 window clipped to the box; kind 3: edge from edges,
 * content = page mask.  edge &= ~content; the first bubble in table order with either bit claims the pixel: edge (255, label, 0),
 * content (0, label, 255); unclaimed pixels are (255, 255, 255).  masks may be NULL when no row has kind 0, page_masks when none has
 * kind 2 or 3, edges when none has kind 0 or 3: the caller vouches for the table, the kernel only keeps its reads inside the planes.
 * init_white != 0 writes the whole page; 0 continues a page, adding bubbles only where it is still white (a claimed pixel is never
 * white, so chunk after chunk onto one page equals one call).  One launch, no host synchronisation; H * W <= 2^30. */
#define VP_BE_PAGE_DESC_INTS 16
int vp_be_compose_page_u8(const float* edges, size_t edge_stride, const float* masks, size_t mask_stride, const int* desc, int m,
                          const unsigned char* page_masks, unsigned char* page, int H, int W, int SH, int SW, float threshold,
                          int init_white, vp_stream stream);

/* ---- evaluation of the mask / edge heads (csrc/seg_eval.hip) ----------------------------------------------------------
 * Per head and image, from logit planes [heads][B][H][W] and target planes of the same shape (fp32, head strides in floats as
 * vp_be_up_infer_f32 takes x_head_stride; any 4-byte-aligned base, 16-byte loads when W % 4 == 0 and bases and strides allow them).
 * The reference has no evaluation (it writes overlays); the loss terms are those of train_BE.py:58-59.  Outputs [heads][B][k]:
 *   sums[4]   {sum bce, sum p t, sum p, sum t}, p = sigmoid(x), bce = max(x, 0) - x t + log1p(exp(-|x|)): vp_be_loss_fwd_f32's
 *   terms[3]  {sum bce / (H W), dice = (2 sum p t + smooth) / (sum p + sum t + smooth), bce_weight * sum bce / (H W) + 1 - dice};
 *             the mean of terms[2] over the images of a head is vp_be_loss_fwd_f32's loss
 *   counts[6] int32 {|P|, |T|, |P & T|, matched_pred, matched_target, nonfinite}: P = (x >= threshold) (a NaN is not in P),
 *             T = (t >= target_threshold); matched_pred = pixels of P with a pixel of T within Chebyshev distance tol inside the same
 *             image, matched_target its mirror image (both |P & T| for tol == 0); nonfinite = logits that are NaN or +-inf
 * tol 0..4, H * W <= 2^24, heads and B <= 65535, finite thresholds; VP_ERR_ARG otherwise, VP_ERR_WORKSPACE for fewer than
 * vp_seg_eval_workspace_bytes() bytes (0 for shapes the entry refuses); ws 8-byte aligned.  Two launches, fixed-order sums (fp64
 * partials), no atomics: two runs give the same bits. */
size_t vp_seg_eval_workspace_bytes(int heads, int B, int H, int W, int tol);
int vp_seg_eval_f32(const float* logits, size_t logit_head_stride, const float* targets, size_t target_head_stride, float* sums,
                    float* terms, int* counts, int heads, int B, int H, int W, float threshold, float target_threshold,
                    float bce_weight, float smooth, int tol, void* ws, size_t ws_bytes, vp_stream stream);

/* ---- inference: the font U-Net, models/networks_BE_font.py ComposeNet in eval mode (csrc/font_infer.hip) ------------
 * vp_conv_in_act_f32: nn.Conv2d(Cin, Cout, ks, stride, padding=(ks-1)/2, bias=False) + nn.InstanceNorm2d(eps) + activation in ONE
 * launch, exact fp32 (v_mfma_f32_16x16x4_f32), for layers whose whole output map fits a 256-row tile.  x NHWC [B][H][W][Cin]; output
 * map Ho x Wo; y[b][p][n] at y + (b*Ho*Wo + p)*ldy + n (ldy >= Cout: y may be a channel slice of a wider NHWC buffer, nothing outside
 * the slice is written); w_packed [Cout][ks*ks][Cin] written by vp_conv_in_pack_f32 from the reference (Cout,Cin,ks,ks) weight.  A
 * workgroup owns 256 / (Ho*Wo) whole images and 16 output channels; per (image, channel): mean over the image's rows, biased variance
 * as the mean of squared deviations from that mean, rstd = 1/sqrt(var + eps), y = act((acc - mean) rstd), act none | relu | lrelu.
 * Image slots of a tile past B are neither read nor written; a result does not depend on the slot or tile its image sits in.
 * vp_conv_in_supported (host only) is the single statement of what the kernel takes: (ks, stride) (3,1) (3,2) (1,1); Ho*Wo 16, 64 or
 * 256 with H, W <= 64; Cin and Cout multiples of 64 up to 1024.  The kernel entry returns VP_ERR_ARG for everything else, and for a
 * null or misaligned (16-byte) x / w_packed, B <= 0, ldy < Cout, another act, and launches nothing.
 * vp_conv_in_preferred (host only) is the subset a plan should use it for: the supported layers with ks*ks*Cin <= 576, where it was
 * measured faster than the convolution + InstanceNorm pair it replaces (DESIGN.md 11.1 has the table). */
int vp_conv_in_supported(int H, int W, int Cin, int Cout, int ks, int stride);
int vp_conv_in_preferred(int H, int W, int Cin, int Cout, int ks, int stride);
int vp_conv_in_pack_f32(const float* w_ref, float* w_packed, int Cout, int Cin, int ks, vp_stream stream);
int vp_conv_in_act_f32(const float* x, const float* w_packed, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int ks, int stride,
                       float eps, int act, float slope, vp_stream stream);
/* The heads' output stage: `heads` Conv2d(C, 1, 3) + bias layers (predictor.2 of edge_net / mask_net) over [heads][B][H][W][C] maps
 * (x_head_stride floats between two heads' maps) in ONE launch; logits [heads][B][H][W]; mask (may be NULL) bytes = logit >= threshold
 * (test_BE_font.py:27-31).  C a multiple of 4 up to 256; head h's parameter block ([9][C] weights, bias; vp_font_pred_params_floats(C)
 * floats, 0 for an unsupported C) starts h blocks in and is written by vp_font_pred_pack_f32 from the (1,C,3,3) weight and the bias. */
size_t vp_font_pred_params_floats(int C);
int vp_font_pred_pack_f32(const float* w, const float* bias, float* params, int C, vp_stream stream);
int vp_font_pred_infer_f32(const float* x, size_t x_head_stride, const float* params, float* logits, unsigned char* mask, float threshold,
                           int heads, int B, int H, int W, int C, vp_stream stream);
/* relay_convs.0's input (models/networks_BE_font.py:214-216): out [B][C*HW + 2E] = [map in (C,H,W) order | label | style] from the
 * NHWC map [B][HW][C] and the two embeddings [B][E]. */
int vp_font_relay_input_f32(const float* map_nhwc, const float* label, const float* style, float* out, int B, int HW, int C, int E,
                            vp_stream stream);
/* SelfAttentionBlock on a 1 x 1 map (models/blocks.py:77-96; the softmax over one position is 1): out = gamma[0] relu(v_pre) + x. */
int vp_font_attn1_f32(const float* v_pre, const float* x, const float* gamma, float* out, size_t n, vp_stream stream);
/* Output-row-stride forms of two existing passes, for producers that write their channel slice of a concatenation's input directly:
 * y row r (an output pixel) starts at y + r*ldy, ldy >= C.  Same arithmetic as vp_upsample2x_bilinear_fwd_f32 /
 * vp_instnorm_act_fwd_f32 (the latter: C % 4 == 0, ldy % 4 == 0, y 16-byte aligned). */
int vp_upsample2x_bilinear_fwd_ld_f32(const float* x, float* y, int ldy, int B, int H, int W, int C, vp_stream stream);
int vp_instnorm_act_fwd_ld_f32(const float* x, float* y, int ldy, float* mean, float* rstd, int B, int R, int C, float eps, int act,
                               float slope, void* ws, size_t ws_bytes, vp_stream stream);

/* ---- SCSEBlock (models/blocks.py:52-65), fp32 NHWC, forward and backward ------------------------------------------------------
 * y[b,p,ch] = x (c[b,ch] + s[b,p]) with the channel gate c = sigmoid(W2 relu(W1 mean_p(x) + b1) + b2) (W1 [C/r][C], W2 [C][C/r], the
 * 1x1 nn.Conv2d weights of cSE.1 / cSE.3 as they are stored) and the spatial gate s = sigmoid(sum_ch w_s[ch] x[b,p,ch] + b_s) (sSE.0);
 * relu != 0 applies the ReLU that follows the block in StyleUp.cat_convs (models/network_Style_GAN.py:54-59) in the same store.
 * Forward reads x twice and writes y once; it leaves pool [B][C] (the means), hid [B][C/r] (after the ReLU), cgate [B][C] and
 * sgate [B][HW] for the backward call.  Backward reads x and dy once, writes dx and adds the pooling term into it in a last pass;
 * the six parameter gradients are written (not accumulated), every sum in a fixed order: no atomics, bit-reproducible.
 * dx may be null: the two stores into dx are then skipped and only the parameter gradients are produced.
 * HW = H * W pixels per image; C <= 1024 when C % 4 == 0 (16-byte accesses), else C <= 256 (scalar accesses).  The 16-byte path
 * needs x, y / dy, dx, cgate, w_s and ws 16-byte aligned; with an unaligned one the scalar path serves C <= 256 and a larger C is
 * refused with VP_ERR_ARG.
 * hidden = C / reduction of the block (>= 1: a block whose C / reduction == 0 is refused).
 * One workspace size serves both calls. */
size_t vp_scse_workspace_bytes(int B, int HW, int C, int hidden);
int vp_scse_fwd_f32(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* w_s,
                    const float* b_s, float* y, float* pool, float* hid, float* cgate, float* sgate, int B, int HW, int C,
                    int hidden, int relu, void* ws, size_t ws_bytes, vp_stream stream);
int vp_scse_bwd_f32(const float* x, const float* dy, const float* w1, const float* w2, const float* w_s, const float* pool,
                    const float* hid, const float* cgate, const float* sgate, float* dx, float* dw1, float* db1, float* dw2,
                    float* db2, float* dw_s, float* db_s, int B, int HW, int C, int hidden, int relu, void* ws,
                    size_t ws_bytes, vp_stream stream);

/* ---- the Style-GAN discriminator's output stage (models/network_Style_GAN.py:214-229), fp32, forward and backward ------------------
 * Two 3x3 stride-2 padding-1 convolutions C -> 1 and C -> K on 2 x 2 maps, then sigmoid and softmax.  Only the taps (i+1, j+1),
 * i, j in {0, 1}, meet data, so per image
 *   adv[b]    = sigmoid(b_adv    + sum_{c,i,j} h_adv[b, 2i+j, c] * w_adv[0, c, i+1, j+1])                       adv [B][1]
 *   aux[b, :] = softmax(b_aux[k] + sum_{c,i,j} h_aux[b, 2i+j, c] * w_aux[k, c, i+1, j+1])  (maximum subtracted)  aux [B][K]
 * h_adv, h_aux: NHWC storage [B][4][C] of the two (B, C, 2, 2) inputs; w_adv (1, C, 3, 3), w_aux (K, C, 3, 3), b_adv [1], b_aux [K] as
 * nn.Conv2d stores them (nothing is packed or copied).  Backward takes adv / aux as the forward call left them and writes (never
 * accumulates) dh_adv, dh_aux [B][4][C], dw_adv (1, C, 3, 3), dw_aux (K, C, 3, 3) with row 0 and column 0 of every 3x3 as 0.0f, db_adv
 * [1], db_aux [K].  d_adv [B][1] or d_aux [B][K] may be null: a zero gradient for that output.  Sums run in a fixed order without
 * atomics (bit-reproducible), in fp32 whatever the convolution precision.  One launch per call, no workspace.
 * Supported: B >= 1, 1 <= C <= 1024, 1 <= K <= 64; anything else, or a null required pointer, is refused with VP_ERR_ARG.  16-byte
 * accesses to h / dh when C % 4 == 0 and those pointers are 16-byte aligned, scalar accesses otherwise (same range). */
int vp_twin_head_fwd_f32(const float* h_adv, const float* h_aux, const float* w_adv, const float* b_adv, const float* w_aux,
                         const float* b_aux, float* adv, float* aux, int B, int C, int K, vp_stream stream);
int vp_twin_head_bwd_f32(const float* h_adv, const float* h_aux, const float* w_adv, const float* w_aux, const float* adv,
                         const float* aux, const float* d_adv, const float* d_aux, float* dh_adv, float* dh_aux, float* dw_adv,
                         float* db_adv, float* dw_aux, float* db_aux, int B, int C, int K, vp_stream stream);

/* ---- SelfAttentionBlock (models/blocks.py:68-96) without the N x N map, exact fp32, forward and backward (csrc/attention.hip,
 * DESIGN.md 11.2).  Per image b: q, k [N][dq]; v, x, g [N][C], row-major (the NHWC memory of the block's maps, N = H * W); dq and C are
 * any positive ints (the block gives dq = C / 8).
 *   forward    o = softmax_rows(q k^T) v,  y = gamma[0] * o + x,  lse[b][i] = log sum_j exp(q_i . k_j)         one launch
 *   backward   dq_out, dk_out, dv_out of y against the upstream gradient g (dx = g is the caller's), dgamma[0] = sum g o; the map is
 *              recomputed from lse, never stored                                                                five launches at most
 * gamma is read on the device.  o and lse are what the backward call needs besides the inputs (gamma may be 0, so o cannot be had
 * from y).  dq_out, dk_out, dv_out may each be null: that gradient's kernel is not launched.  The workspace (delta [B][N] and the
 * partials of dgamma) is vp_attn_bwd_workspace_bytes() bytes, 0 for dims the entry refuses; it grows with B * N alone.
 * Every output element is written by one lane and dgamma is summed from per-workgroup partials in a fixed order: no atomics, no
 * hand-off between workgroups, two runs give the same bits.  16-byte loads when dq % 4 == 0 (q, k) resp. C % 4 == 0 (v, g) and the
 * pointers are 16-byte aligned, 4-byte loads otherwise (same range, same results).
 * VP_ERR_ARG for a non-positive dim, a null required pointer (everything but the three optional gradients), B > 65535, or
 * (N + 64) * max(C, dq) >= 2^31 (the kernels index one image with 32 bits); VP_ERR_WORKSPACE for a workspace that is too small.  A
 * refused call launches nothing. */
int vp_attn_fwd_f32(const float* q, const float* k, const float* v, const float* x, const float* gamma, float* y, float* o, float* lse,
                    int B, int N, int dq, int C, vp_stream stream);
size_t vp_attn_bwd_workspace_bytes(int B, int N, int dq, int C);
int vp_attn_bwd_f32(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* g,
                    const float* gamma, float* dq_out, float* dk_out, float* dv_out, float* dgamma, void* ws, size_t ws_bytes, int B,
                    int N, int dq, int C, vp_stream stream);

/* ---- inference: the Style-GAN row, models/network_Style_GAN.py under torch.no_grad() (csrc/stylegan_infer.hip) ------
 * vp_scse2_fwd_f32: y = relu?(SCSE_b(SCSE_a(x))), two SCSEBlocks of the same C and hidden = C / reduction one after the other (the
 * tail of StyleUp.cat_convs, :54-59), fp32 NHWC [B][HW][C], each block as vp_scse_fwd_f32 defines it; parameters of block a then of
 * block b, as the 1x1 nn.Conv2d weights are stored.  Block a's spatial gate needs no pooling, so block b's pooled input is
 * c_a mean_p(x) + mean_p(x s_a): the call reads x twice and writes y once (two vp_scse_fwd_f32 calls: four reads, two writes) and
 * leaves nothing for a backward call (no pool, hid, cgate, sgate).  y_split (may be NULL; needs C % 8 == 0 and the 16-byte path): the
 * bf16 hi/lo planes of y, plane = B*HW*C elements, laid out as by vp_instnorm_act_fwd_split_f32 and equal to vp_split_f32 of y.
 * Ranges, paths and status codes are vp_scse_fwd_f32's: C <= 1024 when C % 4 == 0 and x, y, w_sa, w_sb, ws are 16-byte aligned, else
 * the scalar path for C <= 256; 1 <= hidden <= C; VP_ERR_ARG for anything else or a null pointer, VP_ERR_WORKSPACE for fewer than
 * vp_scse2_workspace_bytes() bytes; a refused call launches nothing.  Fixed-order sums, no atomics: two runs give the same bits.
 * vp_scse2_preferred (host only): the shapes a plan should take it for over two vp_scse_fwd_f32 calls: C % 4 == 0.
 * vp_cat2_nhwc_f32: out [B][HW][Ca + Cb] = the channel concatenation of a and b; a source is [B][C][HW] (flag 0, NCHW) or
 * [B][HW][C] (flag 1, NHWC).  The generator's input (image, 3 | style plane, 1) and the discriminator's (x, 3 | x_content, 3).
 * vp_sg_out_tanh_f32: Generator.final.3 + tanh (:116-124): out [B][3][H][W] (NCHW) = tanh(Conv2d(C, 3, 3, padding 1)(x) + bias) of
 * the NHWC map x [B][H][W][C], exact fp32, one launch.  C a multiple of 4 up to 256; x and params 16-byte aligned; params
 * ([3][9][C] weights, 3 biases, a zero; vp_sg_out_params_floats(C) floats, 0 for an unsupported C) is written by vp_sg_out_pack_f32
 * from the (3, C, 3, 3) weight and the bias.  vp_sg_out_tanh_preferred (host only): where a plan should take it over the
 * convolution, vp_act_fwd_f32 and vp_nhwc_to_nchw_f32 launches it replaces: C = 32, the width it was measured at. */
size_t vp_scse2_workspace_bytes(int B, int HW, int C, int hidden);
int vp_scse2_preferred(int B, int HW, int C, int hidden);
int vp_scse2_fwd_f32(const float* x, const float* w1a, const float* b1a, const float* w2a, const float* b2a, const float* w_sa,
                     const float* b_sa, const float* w1b, const float* b1b, const float* w2b, const float* b2b, const float* w_sb,
                     const float* b_sb, float* y, void* y_split, int B, int HW, int C, int hidden, int relu, void* ws, size_t ws_bytes,
                     vp_stream stream);
int vp_cat2_nhwc_f32(const float* a, int a_nhwc, const float* b, int b_nhwc, float* out, int B, int HW, int Ca, int Cb, vp_stream stream);
size_t vp_sg_out_params_floats(int C);
int vp_sg_out_tanh_preferred(int B, int H, int W, int C);
int vp_sg_out_pack_f32(const float* w, const float* bias, float* params, int C, vp_stream stream);
int vp_sg_out_tanh_f32(const float* x, const float* params, float* out, int B, int H, int W, int C, vp_stream stream);

/* ---- optimiser step on a flat arena (train_BE.py:62-64,131; train.py:136-140) --------------- */
/* torch.optim.Adam semantics (no amsgrad, no weight decay); g is multiplied by grad_scale first
 * (1/world_size after a sum all-reduce). step is the 1-based step count. */
int vp_adam_f32(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                float eps, int step, float grad_scale, vp_stream stream);
/* The same update for a weight matrix p[R][Cn] whose gradient is a sum of K outer products, g = grad_scale * A^T B (A [K][R] =
 * the output gradients, Bm [K][Cn] = the inputs of a Linear layer, models/networks.py:22,79): the gradient is contracted inside the
 * update and never written.  Replaces the weight-gradient GEMM + vp_adam_f32 on that slice (encoder.fc.0: 134 MB not written
 * and not re-read per step).  R, Cn multiples of 4. */
int vp_adam_outer_f32(float* p, float* m, float* v, const float* A, const float* Bm, int K, int R, int Cn, float lr, float beta1,
                      float beta2, float eps, int step, float grad_scale, vp_stream stream);
/* torch.optim.RMSprop semantics (alpha, eps; no momentum, not centered) */
int vp_rmsprop_f32(float* p, const float* g, float* sq, size_t n, float lr, float alpha, float eps,
                   float grad_scale, vp_stream stream);

#ifdef __cplusplus
}
#endif
#endif
