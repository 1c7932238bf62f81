// Host-only planning of the SelfAttentionBlock kernels (attention.hip): tile sizes, the channel-chunk choice, the workspace layout of
// the backward call and the argument checks.  Nothing here touches the device.
#pragma once
#include "common.h"
#include <cstdint>

namespace vp {
namespace {

constexpr int kAttnTile = 64;          // rows of a stationary tile (16 per wave) and of a swept tile
constexpr int kAttnDK = 32;            // contraction columns staged through LDS at a time
constexpr int kAttnMaxPartials = 1024; // workgroups of the row pass = terms of dgamma's last, serial-per-thread sum

struct AttnPlan {
  int tiles;      // ceil(N / 64): stationary tiles per image
  int nt_c;       // 16-column MFMA tiles per channel chunk of the forward / dV kernels: 4 (chunks of 64) or 8 (chunks of 128)
  int cchunks;    // ceil(C / (16 nt_c))
  int nt_d;       // 16-column tiles per dq chunk of the dK / dQ kernels: 2 (dq <= 32) or 8
  int dchunks;    // ceil(dq / (16 nt_d)): 1 up to dq = 128
  int row_blocks; // workgroups of the row pass (4 rows in flight each)
  size_t ws_delta, ws_partial, ws_floats;   // workspace layout, in floats
};

// Channel chunks of 128 (32 accumulator registers per lane, a 34 KB V tile in LDS: three workgroups per CU) for every C above 64: S is
// recomputed per chunk at dq / 128 of the chunk's own work.  DESIGN.md section 11.2 has the measurement against chunks of 64.
inline AttnPlan attn_plan(int B, int N, int dq, int C) {
  AttnPlan p;
  p.tiles = (N + kAttnTile - 1) / kAttnTile;
  p.nt_c = C <= 64 ? 4 : 8;
  if (const char* e = VP_GETENV("VP_ATTN_NT")) {      // A/B switch of the measurement: 4 | 8
    const int v = atoi(e);
    if (v == 4 || v == 8) p.nt_c = v;
  }
  p.cchunks = (C + 16 * p.nt_c - 1) / (16 * p.nt_c);
  p.nt_d = dq <= 32 ? 2 : 8;
  p.dchunks = (dq + 16 * p.nt_d - 1) / (16 * p.nt_d);
  const size_t rows = (size_t)B * N;
  const size_t rb = (rows + 3) / 4;
  p.row_blocks = (int)(rb < (size_t)kAttnMaxPartials ? rb : (size_t)kAttnMaxPartials);
  p.ws_delta = 0;
  p.ws_partial = (rows + 3) & ~(size_t)3;
  p.ws_floats = p.ws_partial + (((size_t)p.row_blocks + 3) & ~(size_t)3);
  return p;
}

// The kernels index one image with int (row * ld + column) and the batch with size_t; the grid carries the image in z.
inline int attn_check_dims(const char* who, int B, int N, int dq, int C) {
  VP_REQUIRE(B > 0 && N > 0 && dq > 0 && C > 0, "%s: B, N, dq and C must be positive (got %d, %d, %d, %d)", who, B, N, dq, C);
  VP_REQUIRE(B <= 65535, "%s: B = %d exceeds the grid's third dimension", who, B);
  const int64_t widest = C > dq ? C : dq;
  VP_REQUIRE((int64_t)(N + kAttnTile) * widest < ((int64_t)1 << 31),
             "%s: N * max(C, dq) = %lld elements per image overflow the kernels' 32-bit in-image index", who, (long long)N * widest);
  VP_REQUIRE((C + 63) / 64 <= 65535 && (dq + 31) / 32 <= 65535, "%s: C = %d or dq = %d exceeds the grid's second dimension", who, C, dq);
  return VP_OK;
}

}  // namespace
}  // namespace vp
