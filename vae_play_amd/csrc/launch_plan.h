// Launch planning of the split-operand convolutions (bf16x3, f16, the exact-f32 fast path, the inference variants with the affine
// epilogue) and of their weight gradients: route, tile, MFMA form, K-tile depth, split-K, XCD map, phase pairing, and the sizes of
// the statistics and weight-gradient slabs.  Every decision is a pure function of the geometry, a few flags and the A/B switches
// (PlanSwitches, filled by plan_switches() in common.h: nothing here reads the environment) and exists ONCE: a launcher computes a
// plan and executes it, a workspace / support query computes the same plan and reads it.  Host-only (no HIP), so that
// tests/host_emul/plan_emul.cpp pins it on a CPU.  DESIGN.md section 21.
#pragma once
#include <limits.h>
#include "problems.h"
#include "env.h"

namespace vp {

constexpr long WGRAD5_BLOCKS_UNSET = LONG_MIN;
struct PlanSwitches {            // defaults = no variable set
  int igemm16p_mode = 1;         // VP_IGEMM16P: 0 pipelined kernel off, 2 = its 256x256 rule only
  bool igemm16p_m16 = true;      // VP_IGEMM16P_M16
  bool igemm16_m16 = true;       // VP_IGEMM16_M16
  bool wgrad5 = true;            // VP_WGRAD5
  bool wgrad5f = true;           // VP_WGRAD5F
  bool wgrad_pair16 = true;      // VP_WGRAD_PAIR16
  bool f32_fast = true;          // VP_F32_FAST
  long wgrad5_blocks = WGRAD5_BLOCKS_UNSET;      // VP_WGRAD5_BLOCKS
};

// bf16 pairs (three products) | fp16 pairs, two | three products | exact fp32 | fp16 hi planes, one product (inference; planned like
// the other fp16 modes: always ROUTE_STAGED)
enum Arith : int { BF16X3 = 0, F16_2, F16_3, F32, F16_1 };
// LEGACY: fp32 shapes that the fast path refuses (igemm.h; conv.hip asks narrow.hip first)
enum Route : int { ROUTE_LEGACY = 0, ROUTE_HALO, ROUTE_PIPELINED, ROUTE_STAGED };
enum Epilogue : int { EPI_NONE = 0, EPI_STAT, EPI_AFFINE };      // BatchNorm statistics slab | folded BatchNorm (+ ReLU), inference
enum WgradRoute : int { WGRAD_LEGACY = 0, WGRAD_ROWS, WGRAD_WIDE, WGRAD_MAIN };

// tile configurations of the pipelined kernel (igemm16p.h)
enum PCfg : int {
  PCFG_NONE = 0,
  PCFG_128x128_S3,     // 4 waves 2x2, 96 KB: one workgroup per CU
  PCFG_128x128_S2,     // 4 waves 2x2, 64 KB: two workgroups per CU
  PCFG_256x128_S3,     // 8 waves 4x2, 144 KB
  PCFG_256x64_S3,      // 4 waves 4x1, 120 KB
  PCFG_256x64_S2,      // 4 waves 4x1, 80 KB: two per CU
  PCFG_256x256_S2,     // 8 waves 2x4 (wave tile 128x64), 128 KB
  PCFG_128x64_S3,      // 4 waves 2x2 (wave tile 64x32), 72 KB: two per CU
  PCFG_COUNT
};

inline void pcfg_tile(int cfg, int& bm, int& bn) {
  switch (cfg) {
    case PCFG_128x128_S3: case PCFG_128x128_S2: bm = 128; bn = 128; break;
    case PCFG_256x128_S3: bm = 256; bn = 128; break;
    case PCFG_256x64_S3: case PCFG_256x64_S2: bm = 256; bn = 64; break;
    case PCFG_256x256_S2: bm = 256; bn = 256; break;
    case PCFG_128x64_S3: bm = 128; bn = 64; break;
    default: bm = bn = 0;
  }
}

// ---- the rules ------------------------------------------------------------------------------------------------------------------
struct Tile16 { int bm, bn; };   // wave grid: 2 x 2, or 4 x 1 for the 32-column tiles

// Tile of the register-staged kernel (igemm16_kernel).  ctile = the channel count that k is decomposed by, in 16-bit units (the fp32
// path doubles it), 0 for the pixel-major weight gradient.  The fp32 fast path needs >= 64 output columns, so it never sees the
// 32-column tiles (a K-tile is 2.7x more MFMA cycles there, so the same grids are at least as well fed).
inline Tile16 choose_tile16(long M, long N, int gz, int ctile = 0) {
  auto blocks = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn) * (long)gz; };
  const long MINB = 384;      // (per-shape tile searches on the VAE and VAE-GAN steps found nothing beyond noise: profiles/r02_notes.md section 7)
  // a 32-column operand (the 32-channel end of the last decoder block): 64-column tiles would idle half the MFMAs.
  // Unless k runs over 64-channel chunks (ctile = the gathered / scattered side's channel count) and the launch is large: the
  // 32-column tiles exist with 32-deep K-tiles only, and the 64x64 tile on 64-deep FAST K-tiles is 1.4-2.3x faster there even
  // with half of its MFMA columns idle (profiles/r02_g_narrow_n_microbench.log: gather 5x5 s2 64 -> 32 channels 238 -> 106 us, the VAE-GAN
  // discriminator's 64 -> 32 input gradient 252 -> 175 us; 32- and 40-channel chunks keep the narrow tiles: 134 vs 173 us).
  const bool deep = ctile > 0 && ctile % 64 == 0 && (gz == 1 || M * gz >= (1L << 19));
  if (N <= 32 && M >= 128 && !deep) return (M >= 256 && blocks(256, 32) >= MINB) ? Tile16{256, 32} : Tile16{128, 32};
  if (M >= 128 && N >= 128 && blocks(128, 128) >= MINB) return {128, 128};
  if (M >= 128 && N >= 64 && blocks(128, 64) >= MINB) return {128, 64};
  return {64, 64};
}

// XCD-aware tile order (igemm16.h): valid when the row-tile count is a multiple of 8 and there are >= 2 column tiles
inline int xcd_map_tile(long M, long N, int bm, int bn) {
  const long gx = (M + bm - 1) / bm, gy = (N + bn - 1) / bn;
  return (gx % 8 == 0 && gy >= 2) ? 1 : 0;
}

// K-tile depth and FAST (no channel tails) of the gather / scatter families: 64 deep (half the barriers per MFMA) on 64-channel
// chunks, 32 deep on 32-channel chunks (32, 40, 96 ... channels) and on the 32-column tiles (LDS budget: 2-3 workgroups per CU).
// Measured on MI355X, profiles/.
inline void staged_form(int ctile, int bn, int& bk, bool& fast) {
  const bool narrow = bn == 32;      // tiles that exist with 32-deep K-tiles only
  if (ctile > 0 && ctile % 64 == 0 && !narrow) { bk = 64; fast = true; }
  else if (ctile > 0 && ctile % 32 == 0) { bk = 32; fast = true; }
  else { bk = narrow ? 32 : 64; fast = false; }
}
// ... and of the pixel-major weight gradient: 32 deep (its [pixel][channel] LDS images at depth 64 leave one workgroup per CU), FAST
// when the tile lies fully inside M x N.  The two-product fp16 mode stages three planes instead of four: the 64-deep K-tile then
// leaves two workgroups per CU (61 KB each) and halves its barriers (measured -20 us per step, f16x2).
inline void wgrad_form(long M, long N, const Tile16& t, bool x2, int& bk, bool& fast) {
  fast = M % t.bm == 0 && N % t.bn == 0;
  bk = (x2 && t.bn != 32) ? 64 : 32;
}

// layers with fewer output tiles than this split K in two
constexpr long kConvSplitTiles = 384;

// Halo-resident kernels (halo.hip), bf16 pairs only: which plain 5x5 layers they take
inline int halo_gather_kind(int B, int Hs, int Ws, int Cbig, int Csmall, int stride) {
  if (Ws % 16 != 0 || B <= 0) return 0;
  if (Cbig % 32 == 0 && Cbig <= 128 && stride == 1 && Csmall <= 32 && Hs % 16 == 0) return 1;
  if (Cbig == 32 && stride == 2 && Csmall >= 64 && Hs % 8 == 0) return 2;
  if (Cbig == 8 && stride == 2 && Hs % 8 == 0) return 3;
  return 0;
}
inline int halo_scatter_kind(int B, int Hs, int Ws, int Csmall, int /*Cbig*/, int stride) {
  if (stride == 1 && Csmall == 8 && Ws % 16 == 0 && Hs % 16 == 0 && B > 0) return 1;
  return 0;
}

inline bool plain5(const ConvGeom& g) { return g.ks == 5 && g.Hb == g.Hs * g.stride && g.Wb == g.Ws * g.stride; }

// ---- gather and scatter families ---------------------------------------------------------------------------------------------
struct ConvPlan {
  int route = ROUTE_LEGACY;
  int kind = 0;                      // halo kind | PCfg
  int bm = 0, bn = 0, bk = 0;
  bool fast = false, m16 = false;    // no channel tails | the v_mfma_f32_16x16x32_bf16 form
  int nsplit = 1, k_per_split = 0, gz = 1;
  bool zero_fill = false;            // split K: both halves are added atomically onto a zeroed output
  int xcd_map = 0, pair_phases = 0;
  long M = 0, N = 0, K = 0;
  // EPI_STAT: {pivot, sum, sumsq} per (workgroup, channel): stat_floats = 3 * N * stat_tiles_m * gz.  For the fp32 path stat_ok does not
  // look at alignment or operand size (its workspace query never did): the entry points also require route == ROUTE_STAGED.
  bool stat_ok = false; int stat_tiles_m = 0; long stat_R = 0; size_t stat_floats = 0;
  bool affine_ok = false;            // EPI_AFFINE
};

inline ConvPlan plan_conv(bool scatter, const ConvGeom& g, Arith ar, bool has_bias, int act, bool aligned16, int epi, const PlanSwitches& sw) {
  ConvPlan p;
  const bool f32 = ar == F32;
  const int ph = scatter ? g.stride * g.stride : 1;                   // output phases
  const int Cin = scatter ? g.Cs : g.Cb, Cout = scatter ? g.Cb : g.Cs;
  const int C = f32 ? 2 * Cin : Cin;                                  // contracted channels in 16-bit units
  // with a bias the scatter family runs the generic-geometry kernel, whose epilogue adds it
  const bool p5 = plain5(g) && !(scatter && has_bias);
  p.M = scatter ? (long)g.B * g.Hq * g.Wq : (long)g.B * g.Hs * g.Ws;  // the phase grid (problems.h ConvGeom): Hs x Ws for the odd kernels
  p.N = Cout; p.K = (long)g.nt * C;
  const size_t n_in = (size_t)g.B * (scatter ? (size_t)g.Hs * g.Ws : (size_t)g.Hb * g.Wb) * Cin, n_w = (size_t)g.Cs * g.Cb * g.nt;

  if (ar == BF16X3 && p5 && epi != EPI_AFFINE) {
    p.kind = scatter ? halo_scatter_kind(g.B, g.Hs, g.Ws, g.Cs, g.Cb, g.stride) : halo_gather_kind(g.B, g.Hs, g.Ws, g.Cb, g.Cs, g.stride);
    if (p.kind) { p.route = ROUTE_HALO; return p; }
  }

  // split-K: few output tiles and a long K (the 8x8-resolution layers: 256 workgroups = one per CU): split K in two and
  // accumulate both halves with fp32 atomics onto a zeroed output (two addends: the sum does not depend on order, bit-reproducible)
  const long tiles = ((p.M + 127) / 128) * ((p.N + 63) / 64) * ph;
  const bool split = p5 && C % 64 == 0 && tiles < kConvSplitTiles &&
                     (scatter ? 4 * (long)C >= 1024 : (!has_bias && act == ACT_NONE && p.K >= 4096));
  p.nsplit = split ? 2 : 1;
  p.zero_fill = split;
  p.gz = ph * p.nsplit;
  p.k_per_split = (int)(split ? ((p.K / 64 + 1) / 2) * 64 : p.K);

  // Kernel choice for a plain 5x5 VAE layer on split-bf16 planes: the pipelined LDS-DMA kernel (igemm16p.h, bit-identical results) takes
  // the shapes where its 256x256 eight-wave tile fills the chip -- N a multiple of 256 and at least one workgroup per CU, i.e. the
  // N >= 256 layers from ~128 images per GPU on (+5-10 % there, profiles/r02_notes.md); everything else stays on igemm16_kernel.
  // It also takes the small layers and one big gather layer.  VP_IGEMM16P=0 disables it, =2 keeps only the 256x256 rule (A/B).
  // (scatter: stride 2 only; 32-bit byte offsets of both planes; never with the affine epilogue)
  const long kmin = scatter ? (long)ph * C : p.k_per_split;
  int cfg = PCFG_NONE;
  bool pm16 = false;
  if (ar == BF16X3 && p5 && epi != EPI_AFFINE && (!scatter || g.stride == 2) && sw.igemm16p_mode && C % 32 == 0 && kmin / 32 >= 4 &&
      n_in < ((size_t)1 << 29) && n_w < ((size_t)1 << 29)) {
    const int mode = sw.igemm16p_mode;
    if (p.nsplit == 1 && p.N % 256 == 0 && p.M >= 256 && ((p.M + 255) / 256) * (p.N / 256) * p.gz >= 256) cfg = PCFG_256x256_S2;
    // the small layers (8x8 / 16x16 resolution at 32 images: M*N <= 1 M outputs, where igemm16_kernel runs 64x64 / 128x64 tiles with
    // K split in two): the pipelined 128x64 tile, same arithmetic bit for bit, is 4-10 % faster there (r02_a_kbench_m16_b32.log: c7b)
    else if (mode != 2 && p.M * p.N <= (1L << 20) && p.N >= 128 && p.M >= 128) cfg = PCFG_128x64_S3;
    // round 3: the big gather layer where the pipelined kernel on the v_mfma_f32_16x16x32_bf16 form (`m16`) beats igemm16_kernel at 32
    // images (profiles/r02_a_kbench_m16_b32.log: dec2.dgrad 176.0 -> 168.0 us on the 256x128 tile).  Same FLOPs per cycle, but the chip
    // holds a higher clock on this MFMA shape (MI355X_MICROARCH.md, DVFS give-back 7); equal to the 32x32x16 form to rounding, not bit
    // for bit (tests/test_gpu_kbench.py).  Never with the statistics epilogue, which reads the 32x32 accumulator layout
    // (dec2.fwd, the other shape kbench favours, has one).  A/B knob VP_IGEMM16P_M16=0.
    else if (mode != 2 && epi != EPI_STAT && sw.igemm16p_m16 && p.nsplit == 1 && p.gz == 1 && p.N == 256 && p.M >= 16384 && p.M <= 65536 && C == 128) {
      cfg = PCFG_256x128_S3; pm16 = true;
    }
    if (cfg != PCFG_NONE) {
      pcfg_tile(cfg, p.bm, p.bn);
      if (p.bn > p.N || p.bm > p.M) cfg = PCFG_NONE;
    }
  }
  if (cfg != PCFG_NONE) {
    p.route = ROUTE_PIPELINED; p.kind = cfg; p.m16 = pm16;
    p.bk = C % 64 == 0 ? 64 : 32; p.fast = true;
  } else {
    p.route = ROUTE_STAGED;
    const Tile16 t = choose_tile16(p.M, p.N, p.gz, C);
    p.bm = t.bm; p.bn = t.bn;
    staged_form(C, t.bn, p.bk, p.fast);
    // Where the register-staged kernels run their v_mfma_f32_16x16x32_bf16 form (igemm16.h M16; VP_IGEMM16_M16=0: nowhere).
    // Measured per layer in the step at 32 images (profiles/r03_notes.md section 11): the 128x128 tile gains 4 - 5 % in both families
    // (dec1.fwd 180 -> 171 us, dec2.fwd 175 -> 166, dec3.dgrad 174 -> 167), the scatter family's 128x64 tile 2 % on its largest launch
    // (dec3.fwd 239 -> 234); the gather family's 128x64 tile loses 8 % (dec1.dgrad) and the 64x64 tile up to 12 % (enc2.fwd): not taken.
    p.m16 = ar == BF16X3 && p5 && epi != EPI_AFFINE && sw.igemm16_m16 && p.bk == 64 && p.fast && t.bm == 128 &&
            (t.bn == 128 || (scatter && t.bn == 64 && p.M >= 65536));
    // phase pairs (igemm16.h z_setup): a stride-2 scatter of at most two workgroups per CU runs the 9-tap phase beside the 4-tap one
    const long wgs = ((p.M + t.bm - 1) / t.bm) * ((p.N + t.bn - 1) / t.bn) * p.gz;
    p.pair_phases = (scatter && g.stride == 2 && p.nsplit == 1 && wgs <= 512) ? 1 : 0;
  }
  p.xcd_map = xcd_map_tile(p.M, p.N, p.bm, p.bn);

  // the fp32 fast path takes: plain 5x5 layers (big = stride * small), contracted channel count a multiple of 16 (32-deep K-tiles of u16
  // = 16 floats; 64-deep from 32 channels on), at least 64 output columns, 16-B aligned operands, element offsets below 2^31 u16.
  // A/B knob VP_F32_FAST=0: igemm.h for every fp32 convolution.
  const bool f32_shape = sw.f32_fast && Cin % 16 == 0 && Cout >= 64;
  const bool f32_fits = n_in * 2 < ((size_t)1 << 31) && n_w * 2 < ((size_t)1 << 31);
  if (f32 && !(f32_shape && p5 && (scatter || act == ACT_NONE || act == ACT_SIGMOID) && aligned16 && f32_fits)) p.route = ROUTE_LEGACY;

  if (epi == EPI_STAT) {
    p.stat_ok = p.nsplit == 1 && (f32 ? f32_shape : (g.Cb % 8 == 0 && g.Cs % 8 == 0));
    p.stat_tiles_m = (int)((p.M + p.bm - 1) / p.bm);
    p.stat_R = p.M * ph;
    p.stat_floats = p.stat_ok ? (size_t)3 * p.N * p.stat_tiles_m * p.gz : 0;
  }
  // the affine epilogue: K is never split (a non-linear epilogue cannot be applied to partial sums), and only the 32x32 MFMA form on
  // 64-deep channel chunks is instantiated (three tiles per family and arithmetic)
  if (epi == EPI_AFFINE)
    p.affine_ok = Cout >= 64 && Cout % 8 == 0 && C % 64 == 0 && p.nsplit == 1 && p.bn != 32 && (!f32 || (sw.f32_fast && f32_fits));
  return p;
}

// the plans behind the vp_conv5_stats_*_workspace_bytes / vp_conv5_*_stats_* and vp_conv5_affine_supported / vp_conv5_*_affine_* entry points
inline ConvPlan plan_stats(int family, Arith ar, int B, int Hs, int Ws, int Cbig, int Csmall, int stride, bool aligned16, const PlanSwitches& sw) {
  if (B <= 0 || Hs <= 0 || Ws <= 0 || Cbig <= 0 || Csmall <= 0 || (stride != 1 && stride != 2)) return ConvPlan();
  return plan_conv(family != 0, make_geom(B, Hs, Ws, Csmall, Cbig, stride, 5), ar, false, ACT_NONE, aligned16, EPI_STAT, sw);
}
inline ConvPlan plan_affine(int family, int precision, int B, int Hs, int Ws, int Cbig, int Csmall, int stride, const PlanSwitches& sw) {
  if ((family != 0 && family != 1) || precision < 0 || precision > 2) return ConvPlan();      // 0 bf16x3 | 1 f32 | 2 one-product fp16
  if (B <= 0 || Hs <= 0 || Ws <= 0 || Cbig <= 0 || Csmall <= 0 || (stride != 1 && stride != 2)) return ConvPlan();
  return plan_conv(family == 1, make_geom(B, Hs, Ws, Csmall, Cbig, stride, 5), precision == 1 ? F32 : (precision == 2 ? F16_1 : BF16X3), false, ACT_NONE, true,
                   EPI_AFFINE, sw);
}

// ---- weight gradient -----------------------------------------------------------------------------------------------------------
// Row-of-taps kernel (wgrad5.h): plain 5x5 stride-2 layers (Hb = 2*Hs), 128 | Cs, Cb a multiple of 128 or exactly 64,
// K-tiles of 32 pixels that are whole image rows (Ws in {8, 16}) or row segments (32 | Ws), 32-bit element offsets -- every block of
// the VAE / VAE-GAN except the 3-channel edge layers.  A/B knobs VP_WGRAD5=0 / VP_WGRAD5F=0 send them back to the one-tap-per-workgroup kernels.
inline int wgrad5_bn(const ConvGeom& g) {
  if (g.ks != 5 || g.stride != 2 || g.Hb != 2 * g.Hs || g.Wb != 2 * g.Ws) return 0;
  if (g.Cs % 128 != 0) return 0;
  const int bn = g.Cb % 128 == 0 ? 128 : (g.Cb == 64 ? 64 : 0);
  if (!bn) return 0;
  const bool wok = g.Ws % 32 == 0 || g.Ws == 16 || g.Ws == 8;
  if (!wok || ((long)g.Hs * g.Ws) % 32 != 0) return 0;
  if ((size_t)g.B * g.Hb * g.Wb * g.Cb >= ((size_t)1 << 31) || (size_t)g.B * g.Hs * g.Ws * g.Cs >= ((size_t)1 << 31)) return 0;
  return bn;
}

// pixel ranges: one workgroup per CU (the kernel holds 160 accumulators per lane at two waves per SIMD), i.e. ~256 work items
// `items` = work items (= CUs, the kernel owns one per work item) the launch may take; <= 0: the whole chip.  A caller that runs the
// weight gradient beside other kernels leaves part of the chip to them: on the side stream of the fused step ~5/8 of the chip is
// the measured optimum (step 3.588 ms with the one-tap kernels; rows of taps with 256 work items 3.52, 176: 3.479, 160: 3.455,
// 144: 3.471, 128: 3.484, 96: 3.67 -- profiles/r03_notes.md): the main stream's kernels keep the rest instead of queueing behind
// one-workgroup-per-CU launches, and the slabs shrink with the count.
// A budget above the chip's WGRAD5_MAX_ITEMS CUs (MI355X: 256) means nothing more and is clamped to it: the workspace queries size
// the slabs for items = 0, i.e. WGRAD5_MAX_ITEMS, so a larger count would split K deeper than the queried workspace holds.
// `blocks` (VP_WGRAD5_BLOCKS, A/B): overrides the caller's count.
constexpr int WGRAD5_MAX_ITEMS = 256;
inline int wgrad5_split(const ConvGeom& g, int bn, int items, long blocks, int* k_per_split) {
  const long K = (long)g.B * g.Hs * g.Ws;
  const long inner = (long)(g.Cs / 128) * (g.Cb / bn) * 5;
  long target = items > 0 && items < WGRAD5_MAX_ITEMS ? items : WGRAD5_MAX_ITEMS;
  if (blocks != WGRAD5_BLOCKS_UNSET) target = blocks;
  long ns = target / inner;
  if (ns < 1) ns = 1;
  const long maxs = K / 128 > 0 ? K / 128 : 1;                               // at least four K-tiles per split
  if (ns > maxs) ns = maxs;
  long per = ((K + ns - 1) / ns + 31) / 32 * 32;
  ns = (K + per - 1) / per;                                                  // no empty split
  *k_per_split = (int)per;
  return (int)ns;
}
inline size_t wgrad5_slab_floats(const ConvGeom& g, int bn, int ns) { return (size_t)ns * (bn == 64 ? 2 : 1) * 25 * g.Cs * g.Cb; }

// Tap pairs (ProbW16T<.., PAIR>, igemm16.h): a 5x5 or 3x3 layer whose big side has 32 or 64 channels contracts TWO taps per workgroup, the
// two taps' channels side by side in a 64- / 128-column tile: a 32-channel layer no longer pads half of a 64-column tile (and leaves the
// slow partial-tile loads), a 64-channel layer gets a 128-column tile's operand reuse.  (nt + 1) / 2 pairs instead of nt taps per split:
// the pixel range is split twice as deep where the workspace allows.  A 64-channel SMALL side takes the 64x128 tile (wave tiles
// 32x64) instead of 64x64 (32x32): with 128 | 256 | ... big channels directly (kind 4), with 64 big channels on tap pairs (kind 3) --
// the font U-Net's full-resolution layers, 110 -> ~170 TFLOP/s (tools/microbench_font_layers.py).
//   kind 1: pairs, 64x64 tile (Cb = 32) | 2: pairs, 128x128 (Cb = 64, Cs % 128 == 0) | 3: pairs, 64x128 (Cb = 64, Cs % 64 == 0)
//   kind 4: single taps, 64x128 tile (Cs % 128 == 64, Cb % 128 == 0)
inline int wgrad_wide_kind(const ConvGeom& g, bool pair16) {
  // 16 taps (the 4x4 layers of models/network_Style_GAN.py:49,95-98,116) pair without a remainder; A/B knob VP_WGRAD_PAIR16=0 sends
  // them back to single taps
  const bool pair_nt = g.nt == 25 || g.nt == 9 || (g.nt == 16 && pair16);
  if (pair_nt && g.Cb == 32 && g.Cs % 64 == 0) return 1;
  if (pair_nt && g.Cb == 64 && g.Cs % 128 == 0) return 2;
  if (pair_nt && g.Cb == 64 && g.Cs % 64 == 0) return 3;
  if (g.Cs % 128 == 64 && g.Cb % 128 == 0) return 4;
  return 0;
}
inline int wgrad_pair_nsplit(const ConvGeom& g, int ns) {
  const long K = (long)g.B * g.Hs * g.Ws, maxs = (K + 511) / 512;
  long n2 = 2L * ns;
  if (n2 > maxs) n2 = maxs;
  if (n2 > 64) n2 = 64;
  return n2 > ns ? (int)n2 : ns;
}

struct WgradPlan {
  int route = WGRAD_LEGACY;          // LEGACY: fp32 on igemm.h (conv.hip asks narrow.hip first)
  int kind = 0;                      // ROWS: big-channel tile 64 | 128; WIDE: 1-4
  int bm = 0, bn = 0, bk = 0; bool fast = false;      // WIDE and MAIN
  int N = 0, gz = 0;                 // WIDE and MAIN: columns (tap pairs: 2 * Cb) and grid depth
  int nsplit = 1, k_per_split = 0, slabs = 1;         // slabs: what the fixed-order reduction sums
  size_t slab_floats = 0;            // what the launch writes
  size_t need_floats = 0;            // the smallest workspace the launcher accepts
  size_t query_floats = 0;           // what *_wgrad*_workspace_bytes reports: holds every max_cus, and the deeper split of tap pairs
};

// ws_bytes: the caller's workspace (tap pairs split twice as deep when it holds that); max_cus: work-item budget of the rows of taps
inline WgradPlan plan_wgrad(const ConvGeom& g, Arith ar, int max_cus, size_t ws_bytes, bool aligned16, const PlanSwitches& sw) {
  WgradPlan w;
  const bool f32 = ar == F32;
  const long K = (long)g.B * g.Hs * g.Ws;
  const int ns = wgrad_nsplit(g);
  const int wide = ar == BF16X3 ? wgrad_wide_kind(g, sw.wgrad_pair16) : 0;
  const int ns2 = wgrad_pair_nsplit(g, ns);
  // the query: the one-tap kernels' slabs (tap pairs: at their deeper split; the fp16 modes share the split-bf16 query), or one
  // slab set per CU-filling round of the rows of taps (the fp32 query does not look at its switch or at alignment)
  const int pairs = f32 ? 0 : wgrad_wide_kind(g, sw.wgrad_pair16);
  w.query_floats = wgrad_slab_floats(g, (pairs >= 1 && pairs <= 3) ? ns2 : ns);
  int kper = 0;
  if (const int bnq = (f32 || sw.wgrad5) ? wgrad5_bn(g) : 0) {
    const size_t n5 = wgrad5_slab_floats(g, bnq, wgrad5_split(g, bnq, 0, sw.wgrad5_blocks, &kper));
    if (n5 > w.query_floats) w.query_floats = n5;
  }
  if (const int bn = (f32 ? (sw.wgrad5f && aligned16) : sw.wgrad5) ? wgrad5_bn(g) : 0) {
    w.route = WGRAD_ROWS; w.kind = bn; w.bm = 128; w.bn = bn;
    w.nsplit = wgrad5_split(g, bn, max_cus, sw.wgrad5_blocks, &kper);
    w.k_per_split = kper;
    w.slabs = w.nsplit * (bn == 64 ? 2 : 1);
    w.slab_floats = w.need_floats = wgrad5_slab_floats(g, bn, w.nsplit);
  } else {
    w.need_floats = wgrad_slab_floats(g, ns);
    w.nsplit = ns;
    if (wide) {
      // deeper split when the caller's workspace holds it (the *_workspace_bytes query asks for it)
      if (wide <= 3 && ws_bytes / sizeof(float) >= wgrad_slab_floats(g, ns2)) w.nsplit = ns2;
      w.route = WGRAD_WIDE; w.kind = wide;
      w.bm = wide == 2 ? 128 : 64; w.bn = wide == 1 ? 64 : 128; w.bk = 32; w.fast = true;
      w.N = wide == 4 ? g.Cb : 2 * g.Cb;
      w.gz = (wide == 4 ? g.nt : (g.nt + 1) / 2) * w.nsplit;
    } else if (!f32) {
      w.route = WGRAD_MAIN;
      w.N = g.Cb; w.gz = g.nt * ns;
      const Tile16 t = choose_tile16(g.Cs, g.Cb, w.gz);
      w.bm = t.bm; w.bn = t.bn;
      wgrad_form(g.Cs, g.Cb, t, ar == F16_2, w.bk, w.fast);
    }
    w.slabs = w.nsplit;
    w.slab_floats = wgrad_slab_floats(g, w.nsplit);
    w.k_per_split = (int)(((K + w.nsplit - 1) / w.nsplit + 31) / 32 * 32);
  }
  if (f32 && w.query_floats > w.need_floats) w.need_floats = w.query_floats;      // conv.hip has always asked for the whole query
  return w;
}

}  // namespace vp
