// Fused eval-mode inference of the font U-Net (models/networks_BE_font.py ComposeNet): what the whole-image convolution +
// InstanceNorm kernel of font_infer.hip takes, stated once in host-only code (vp_conv_in_supported is this predicate; the kernel
// entry refuses what it refuses), and the layout of the heads' output-stage parameter block.  DESIGN.md 11.1.
#pragma once

namespace vp {
namespace font {

constexpr int TILE_ROWS = 256;   // output rows (pixels) a workgroup owns: 256 / (Ho * Wo) whole images
constexpr int TILE_CH = 16;      // output channels a workgroup owns: one column of v_mfma_f32_16x16x4_f32 tiles
constexpr int SLICE_K = 32;      // K elements per LDS slice; Cin % 64 == 0 keeps a slice inside one filter tap
constexpr int MAX_CIN = 1024, MAX_COUT = 1024;

struct ConvInGeom {
  int Ho, Wo, pad, pixels, images;   // output map, padding, Ho * Wo, whole images per tile
};

// nn.Conv2d(Cin, Cout, ks, stride, padding=(ks-1)//2, bias=False) on an H x W input whose whole output map fits a tile
inline bool conv_in_geom(int H, int W, int ks, int stride, ConvInGeom& g) {
  const bool kind = (ks == 3 && (stride == 1 || stride == 2)) || (ks == 1 && stride == 1);
  if (!kind || H <= 0 || W <= 0 || H > 64 || W > 64) return false;
  g.pad = (ks - 1) / 2;
  g.Ho = (H + 2 * g.pad - ks) / stride + 1;
  g.Wo = (W + 2 * g.pad - ks) / stride + 1;
  g.pixels = g.Ho * g.Wo;
  if (g.pixels != 16 && g.pixels != 64 && g.pixels != 256) return false;
  g.images = TILE_ROWS / g.pixels;
  return true;
}

inline bool conv_in_supported(int H, int W, int Cin, int Cout, int ks, int stride) {
  ConvInGeom g;
  if (!conv_in_geom(H, W, ks, stride, g)) return false;
  if (Cin < 64 || Cin > MAX_CIN || Cin % 64 != 0) return false;
  return Cout >= 64 && Cout <= MAX_COUT && Cout % 64 == 0;
}

// Where a plan should USE the kernel: the layers it was measured faster on than the convolution + InstanceNorm pair it replaces
// (MI355X, batch 16).  Its time grows with K = ks * ks * Cin alone, 1.39 us per 32-deep K slice against the pair's
// 1.05 us per slice plus ~10 us for the InstanceNorm pass: faster at K = 256 (15.1 against 19.9 us) and K = 576 (29.5 against 30.6 us),
// slower from K = 1152 (53.8 against 48.2 us) up to K = 9216 (398 against 293 us).
constexpr int PREFER_MAX_K = 576;
inline bool conv_in_preferred(int H, int W, int Cin, int Cout, int ks, int stride) {
  return conv_in_supported(H, W, Cin, Cout, ks, stride) && ks * ks * Cin <= PREFER_MAX_K;
}

// output stage of the two heads (Conv2d(C, 1, 3) + bias): per head [9][C] weights (tap-major, channel contiguous), then the bias
// padded to four floats
#ifdef __HIPCC__
#define VP_FONT_HD __host__ __device__
#else
#define VP_FONT_HD
#endif
inline bool pred_supported(int C) { return C >= 4 && C <= 256 && C % 4 == 0; }
VP_FONT_HD inline int pred_params_floats(int C) { return 9 * C + 4; }

}  // namespace font
}  // namespace vp
