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

}  // namespace vp
