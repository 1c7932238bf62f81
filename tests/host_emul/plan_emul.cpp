// Host build of the launch planner (vae_play_amd/csrc/launch_plan.h) for tests/test_launch_plan.py: every plan field as int64.
// Compiled on demand with the ROCm clang++ (no HIP); the switches are passed by value, nothing here reads the environment.
#include <stdint.h>
#include "../../vae_play_amd/csrc/launch_plan.h"

using namespace vp;

namespace vp { const void* vp_zero_page() { return nullptr; } }      // (declared by problems.h; never called here)

// sw: {igemm16p_mode, igemm16p_m16, igemm16_m16, wgrad5, wgrad5f, wgrad_pair16, f32_fast, wgrad5_blocks or INT64_MIN = unset}
static PlanSwitches switches(const int64_t* sw) {
  PlanSwitches s;
  if (!sw) return s;
  s.igemm16p_mode = (int)sw[0]; s.igemm16p_m16 = sw[1] != 0; s.igemm16_m16 = sw[2] != 0; s.wgrad5 = sw[3] != 0; s.wgrad5f = sw[4] != 0;
  s.wgrad_pair16 = sw[5] != 0; s.f32_fast = sw[6] != 0;
  s.wgrad5_blocks = sw[7] == INT64_MIN ? WGRAD5_BLOCKS_UNSET : (long)sw[7];
  return s;
}

static void put(const ConvPlan& p, int64_t* o) {
  const int64_t v[] = {p.route, p.kind, p.bm, p.bn, p.bk, p.fast, p.m16, p.nsplit, p.k_per_split, p.gz, p.zero_fill, p.xcd_map, p.pair_phases,
                       p.M, p.N, p.K, p.stat_ok, p.stat_tiles_m, p.stat_R, (int64_t)p.stat_floats, p.affine_ok};
  for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) o[i] = v[i];
}

extern "C" {

int vp_plan_conv_fields() { return 21; }
int vp_plan_wgrad_fields() { return 14; }

void vp_plan_conv(int scatter, int arith, int B, int Hs, int Ws, int Hb, int Wb, int Cbig, int Csmall, int ks, int stride, int has_bias, int act,
                  int aligned16, int epi, const int64_t* sw, int64_t* out) {
  put(plan_conv(scatter != 0, make_geom(B, Hs, Ws, Csmall, Cbig, stride, ks, Hb, Wb), (Arith)arith, has_bias != 0, act, aligned16 != 0, epi, switches(sw)), out);
}

void vp_plan_stats(int family, int arith, int B, int Hs, int Ws, int Cbig, int Csmall, int stride, int aligned16, const int64_t* sw, int64_t* out) {
  put(plan_stats(family, (Arith)arith, B, Hs, Ws, Cbig, Csmall, stride, aligned16 != 0, switches(sw)), out);
}

void vp_plan_affine(int family, int precision, int B, int Hs, int Ws, int Cbig, int Csmall, int stride, const int64_t* sw, int64_t* out) {
  put(plan_affine(family, precision, B, Hs, Ws, Cbig, Csmall, stride, switches(sw)), out);
}

// ws_bytes < 0: SIZE_MAX (what the workspace queries pass)
void vp_plan_wgrad(int arith, int B, int Hs, int Ws, int Hb, int Wb, int Cbig, int Csmall, int ks, int stride, int max_cus, int64_t ws_bytes,
                   int aligned16, const int64_t* sw, int64_t* out) {
  const WgradPlan w = plan_wgrad(make_geom(B, Hs, Ws, Csmall, Cbig, stride, ks, Hb, Wb), (Arith)arith, max_cus,
                                 ws_bytes < 0 ? SIZE_MAX : (size_t)ws_bytes, aligned16 != 0, switches(sw));
  const int64_t v[] = {w.route, w.kind, w.bm, w.bn, w.bk, w.fast, w.N, w.gz, w.nsplit, w.k_per_split, w.slabs, (int64_t)w.slab_floats,
                       (int64_t)w.need_floats, (int64_t)w.query_floats};
  for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}

}
