// Shared host-side plumbing for the C ABI: status codes, thread-local error text, checks.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdarg>
#include <cstdint>
#include "../../include/vaeplay_hip.h"
#include "env.h"
#include "launch_plan.h"

namespace vp {

inline char* err_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(VP_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return VP_OK;
}

#define VP_REQUIRE(cond, ...)                                 \
  do {                                                        \
    if (!(cond)) return ::vp::fail(VP_ERR_ARG, __VA_ARGS__);  \
  } while (0)

// The A/B switches of the launch planner (launch_plan.h), looked up as each knob always was: VP_IGEMM16P and VP_IGEMM16P_M16 once per
// process, the others through VP_GETENV (cached per process unless VP_ENV_DYNAMIC=1).  DESIGN.md section 13.
inline PlanSwitches plan_switches() {
  static const int p_mode = [] { const char* e = getenv("VP_IGEMM16P"); return e ? atoi(e) : 1; }();
  static const bool p_m16 = [] { const char* e = getenv("VP_IGEMM16P_M16"); return !e || atoi(e) != 0; }();
  auto on = [](const char* e) { return !(e && atoi(e) == 0); };
  PlanSwitches sw;
  sw.igemm16p_mode = p_mode;
  sw.igemm16p_m16 = p_m16;
  sw.igemm16_m16 = on(VP_GETENV("VP_IGEMM16_M16"));
  sw.wgrad5 = on(VP_GETENV("VP_WGRAD5"));
  sw.wgrad5f = on(VP_GETENV("VP_WGRAD5F"));
  sw.wgrad_pair16 = on(VP_GETENV("VP_WGRAD_PAIR16"));
  sw.f32_fast = on(VP_GETENV("VP_F32_FAST"));
  if (const char* e = VP_GETENV("VP_WGRAD5_BLOCKS")) sw.wgrad5_blocks = atol(e);
  return sw;
}

// every pointer is 16-byte aligned (a null pointer counts as aligned)
template <class... T>
inline bool aligned16(const T*... p) { return ((... | (uintptr_t)p) & 15) == 0; }

inline unsigned grid_for(size_t work_items, int block, unsigned cap = 256 * 8) {
  size_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

// wave64 sum via DPP-free shuffles (64-lane wavefront)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) { return wave_sum_d(v); }

// Sum over a 256-thread workgroup (four waves), returned to every thread: the wave tree, then (sh[0] + sh[1]) + (sh[2] + sh[3]).
// sh holds four values; a kernel with several accumulators calls this once per accumulator, each with four values of its own.
// The one fixed order of every block sum of the small kernels (elementwise.hip, score.h).  The serial sums of
// cross_entropy_fwd_kernel (256 entries), l1_final_kernel and be_loss_final_kernel have other orders and stay as they are.
template <class T>
__device__ __forceinline__ T block_sum4(T lane_value, T* sh) {
  const T w = wave_sum(lane_value);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- loss terms stated once -------------------------------------------------------------------------------------------------------
// F.binary_cross_entropy's term t log p + (1 - t) log(1 - p) with torch's clamp of each logarithm at -100; the callers subtract it
// (reduce_partial_kernel<0> of elementwise.hip, bce_rows_kernel of score.h)
__device__ __forceinline__ float bce_term(float p, float t) {
  const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(logf(1.f - p), -100.f);
  return t * lp + (1.f - t) * lq;
}

// p = sigmoid(x) and q = 1 - p = sigmoid(-x), each from e = exp(-|x|), which the caller computes (expf in the GAN head, __expf in
// the BE kernels): "1.f - p" loses q once p rounds towards 1
__device__ __forceinline__ void sigmoid_pair(float x, float e, float& p, float& q) {
  const float big = 1.f / (1.f + e), small = e / (1.f + e);
  p = x >= 0.f ? big : small;
  q = x >= 0.f ? small : big;
}

// -log(p + 1e-3) of a probability p with q = 1 - p from sigmoid_pair (VaeGan.loss, models/networks.py:274-276), every value relative
// to itself: towards p = 1 the sum p + 1e-3 rounds at 6e-8 next to a result of -1e-3 -- 5e-5 of it -- so that side is formed as
// -log1p(1e-3 - q).  The other side is the expression of the training step's GAN head (gan_head_kernel, whose bits stay as they are).
__device__ __forceinline__ float neg_log_floor(float p, float q) {
  return p <= 0.5f ? -logf(p + 1e-3f) : -log1pf(1e-3f - q);
}

// ---- host launch sequences stated once ---------------------------------------------------------------------------------------------
// a flat kernel of 256-thread workgroups over `items` work items, its grid capped at `cap` workgroups (grid_for)
constexpr unsigned FLAT_CAP = 256 * 8;
template <class... K, class... A>
inline int launch_flat(const char* what, void (*kernel)(K...), size_t items, unsigned cap, hipStream_t s, A... args) {
  hipLaunchKernelGGL(kernel, dim3(grid_for(items, 256, cap)), dim3(256), 0, s, static_cast<K>(args)...);
  return check_launch(what);
}

// the two-stage reductions: the workspace check with the caller's message, the partial launch, the final launch
template <class Partial, class Final>
inline int two_stage(const char* what, bool ws_ok, const char* ws_message, Partial partial, Final final) {
  if (!ws_ok) return fail(VP_ERR_WORKSPACE, "%s: %s", what, ws_message);
  auto check = [what](const char* stage) {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? (int)VP_OK : fail(VP_ERR_LAUNCH, "%s(%s): %s", what, stage, hipGetErrorString(e));
  };
  partial();
  if (int rc = check("partial")) return rc;
  final();
  return check("final");
}

}  // namespace vp
