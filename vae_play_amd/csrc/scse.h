// What the SCSEBlock kernels share (scse.hip: forward and backward of one block; stylegan_infer.hip: two blocks in one pass pair):
// the chunk plan, the float4 / float element helpers, the pixel-slot butterfly, the instantiation table and the argument checks.
// Everything is internal to the translation unit that includes it.
#pragma once
#include "common.h"
#include <cstdint>

namespace vp {
namespace {

constexpr int kScseMaxC = 1024;      // LDS vectors of the gate kernels, and 64 lanes * 4 float4 per pixel slot
constexpr int kScseMaxCScalar = 256; // the scalar path holds 64 lanes * 4 floats per pixel slot

struct ScsePlan {
  int ppc;        // pixels per chunk
  int nchunk;     // chunks per image
};

// Chunks of at least 32 KB of x (the two partial rows a workgroup writes in backward are then at most 1/16 of one pass), and no more
// chunks than give ~2048 workgroups over the batch (8 per CU); at most 256 per image so that the gate kernels' serial sums stay short.
inline ScsePlan scse_plan(int B, int HW, int C) {
  int maxchunks = 2048 / B;
  maxchunks = maxchunks < 1 ? 1 : (maxchunks > 256 ? 256 : maxchunks);
  int ppc = (HW + maxchunks - 1) / maxchunks;
  const int ppc_min = 8192 / C > 1 ? 8192 / C : 1;
  if (ppc < ppc_min) ppc = ppc_min;
  return {ppc, (HW + ppc - 1) / ppc};
}

// ---- element helpers: one code path for float4 and float ----------------------------------------------------------------------
__device__ __forceinline__ void zero(float& a) { a = 0.f; }
__device__ __forceinline__ void zero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float mul(float a, float b) { return a * b; }
__device__ __forceinline__ float4 mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float adds(float a, float s) { return a + s; }
__device__ __forceinline__ float4 adds(float4 a, float s) { return make_float4(a.x + s, a.y + s, a.z + s, a.w + s); }
__device__ __forceinline__ float muls(float a, float s) { return a * s; }
__device__ __forceinline__ float4 muls(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float dot(float a, float b) { return a * b; }
__device__ __forceinline__ float dot(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
// torch.relu's values: a NaN stays a NaN (fmaxf would turn it into 0 and hide it)
__device__ __forceinline__ float relu(float a) { return a < 0.f ? 0.f : a; }
__device__ __forceinline__ float4 relu(float4 a) { return make_float4(relu(a.x), relu(a.y), relu(a.z), relu(a.w)); }
// dy where x > 0, else 0: the mask of the fused ReLU (y = x (c + s) with c + s > 0, so y > 0 exactly where x > 0)
__device__ __forceinline__ float mask_pos(float g, float x) { return x > 0.f ? g : 0.f; }
__device__ __forceinline__ float4 mask_pos(float4 g, float4 x) {
  return make_float4(x.x > 0.f ? g.x : 0.f, x.y > 0.f ? g.y : 0.f, x.z > 0.f ? g.z : 0.f, x.w > 0.f ? g.w : 0.f);
}
__device__ __forceinline__ float sigmoidf(float z) {
  const float e = expf(-fabsf(z));
  return z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
// sum over the G lanes of a pixel slot (G a power of two, slots are aligned runs of lanes): every lane ends with the same bits
template <int G>
__device__ __forceinline__ float slot_sum(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// picks the instantiation whose G * K lanes-times-elements cover `nel` elements per pixel
#define SCSE_DISPATCH(T, nel, LAUNCH) \
  do {                                \
    if ((nel) <= 4) {                 \
      LAUNCH(T, 4, 1);                \
    } else if ((nel) <= 8) {          \
      LAUNCH(T, 8, 1);                \
    } else if ((nel) <= 16) {         \
      LAUNCH(T, 16, 1);               \
    } else if ((nel) <= 32) {         \
      LAUNCH(T, 32, 1);               \
    } else if ((nel) <= 64) {         \
      LAUNCH(T, 64, 1);               \
    } else if ((nel) <= 128) {        \
      LAUNCH(T, 64, 2);               \
    } else {                          \
      LAUNCH(T, 64, 4);               \
    }                                 \
  } while (0)

inline int scse_check_dims(const char* who, int B, int HW, int C, int Cr) {
  VP_REQUIRE(B > 0 && HW > 0 && C > 0, "%s: B, HW and C must be positive", who);
  VP_REQUIRE(Cr > 0 && Cr <= C, "%s: hidden = %d channels (C / reduction == 0, or more than C = %d): the channel gate needs 1 <= hidden <= C",
             who, Cr, C);
  VP_REQUIRE(C <= kScseMaxC && (C % 4 == 0 || C <= kScseMaxCScalar), "%s: C = %d is not supported (C <= %d when C %% 4 == 0, else C <= %d)",
             who, C, kScseMaxC, kScseMaxCScalar);
  VP_REQUIRE(B <= 65535, "%s: B = %d exceeds the grid's second dimension", who, B);
  return VP_OK;
}

// the scalar path stands in for the float4 path when a pointer is not 16-byte aligned, but only as far as it reaches
inline int scse_check_path(const char* who, bool vec, int C) {
  VP_REQUIRE(vec || C <= kScseMaxCScalar, "%s: C = %d needs 16-byte aligned tensors and workspace (unaligned pointers are served up to C = %d)",
             who, C, kScseMaxCScalar);
  return VP_OK;
}

}  // namespace
}  // namespace vp
