"""The launch planner (vae_play_amd/csrc/launch_plan.h) on a CPU: tests/host_emul/plan_emul.cpp is the header compiled for the host.

  1. the workspace / support queries that read the plan return what the library returned before the planner existed
     (tests/golden/conv_launch_plans.json, recorded by tools/gen_golden_launch_plans.py from the parent's library), at every point of
     the shape grid; where the file holds launches recorded on an MI355X, the kernel and grid derived from the plan equal them;
  2. invariants of every plan over the same grid;
  3. each A/B switch, flipped by value, changes the routes DESIGN.md section 13 says it changes;
  4. the shapes of tests/test_gpu_launch_plan_branches.py still take the branch they are listed for."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_emul", "plan_emul.cpp")
OUT = os.path.join(HERE, "host_emul", "libvp_plan_emul.so")
CSRC = os.path.join(ROOT, "vae_play_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "conv_launch_plans.json")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_launch_plans as G  # noqa: E402  (the grid and the argument order of every query)

BF16X3, F16_2, F16_3, F32 = range(4)
LEGACY, HALO, PIPELINED, STAGED = range(4)
EPI_NONE, EPI_STAT, EPI_AFFINE = range(3)
W_LEGACY, W_ROWS, W_WIDE, W_MAIN = range(4)
PCFG = {3: (256, 128), 6: (256, 256), 7: (128, 64)}          # the pipelined configurations the library instantiates
CONV_FIELDS = ("route kind bm bn bk fast m16 nsplit k_per_split gz zero_fill xcd_map pair_phases M N K stat_ok stat_tiles_m stat_R "
               "stat_floats affine_ok").split()
WGRAD_FIELDS = "route kind bm bn bk fast N gz nsplit k_per_split slabs slab_floats need_floats query_floats".split()
SWITCHES = "igemm16p_mode igemm16p_m16 igemm16_m16 wgrad5 wgrad5f wgrad_pair16 f32_fast wgrad5_blocks".split()
I64 = ctypes.c_int64


class Plan(dict):
    __getattr__ = dict.__getitem__


class Planner:
    def __init__(self, lib):
        self.lib = lib
        assert lib.vp_plan_conv_fields() == len(CONV_FIELDS) and lib.vp_plan_wgrad_fields() == len(WGRAD_FIELDS)
        self.cbuf, self.wbuf = (I64 * len(CONV_FIELDS))(), (I64 * len(WGRAD_FIELDS))()
        lib.vp_plan_wgrad.argtypes = [ctypes.c_int] * 11 + [I64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]

    @staticmethod
    def _sw(switches):
        if not switches:
            return None
        v = dict(igemm16p_mode=1, igemm16p_m16=1, igemm16_m16=1, wgrad5=1, wgrad5f=1, wgrad_pair16=1, f32_fast=1, wgrad5_blocks=-2 ** 63)
        v.update(switches)
        return (I64 * 8)(*(int(v[k]) for k in SWITCHES))

    def conv(self, scatter, arith, B, Hs, Ws, Cbig, Csmall, stride, ks=5, Hb=0, Wb=0, has_bias=0, act=0, aligned16=1, epi=EPI_NONE, sw=None):
        self.lib.vp_plan_conv(int(scatter), arith, B, Hs, Ws, Hb, Wb, Cbig, Csmall, ks, stride, has_bias, act, aligned16, epi, self._sw(sw),
                              self.cbuf)
        return Plan(zip(CONV_FIELDS, self.cbuf))

    def stats(self, family, arith, B, Hs, Ws, Cbig, Csmall, stride, sw=None):
        self.lib.vp_plan_stats(family, arith, B, Hs, Ws, Cbig, Csmall, stride, 1, self._sw(sw), self.cbuf)
        return Plan(zip(CONV_FIELDS, self.cbuf))

    def affine(self, family, precision, B, Hs, Ws, Cbig, Csmall, stride, sw=None):
        self.lib.vp_plan_affine(family, precision, B, Hs, Ws, Cbig, Csmall, stride, self._sw(sw), self.cbuf)
        return Plan(zip(CONV_FIELDS, self.cbuf))

    def wgrad(self, arith, B, Hs, Ws, Hb, Wb, Cbig, Csmall, ks, stride, max_cus=0, ws_bytes=-1, aligned16=1, sw=None):
        self.lib.vp_plan_wgrad(arith, B, Hs, Ws, Hb, Wb, Cbig, Csmall, ks, stride, max_cus, ws_bytes, aligned16, self._sw(sw), self.wbuf)
        return Plan(zip(WGRAD_FIELDS, self.wbuf))


def load_planner():
    hdrs = [os.path.join(CSRC, h) for h in ("launch_plan.h", "problems.h", "env.h")]
    if (not os.path.exists(OUT)) or os.path.getmtime(OUT) < max(map(os.path.getmtime, [SRC] + hdrs)):
        cxx = "/opt/rocm/lib/llvm/bin/clang++"
        if not os.path.exists(cxx):
            cxx = "clang++"
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", OUT])
    return Planner(ctypes.CDLL(OUT))


@pytest.fixture(scope="module")
def planner():
    return load_planner()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def ceil_div(a, b):
    return -(-a // b)


# ---- 1. the queries against the parent's library --------------------------------------------------------------------------------------
def _narrow_wgrad(p):
    """the fp32 weight gradients that conv.hip hands to narrow.hip before it plans (narrow_wgrad_kind: not a planner rule)"""
    Cb, Cs = p["Cbig"], p["Csmall"]
    return p["ks"] == 5 and ((p["stride"] == 1 and Cs in (1, 3) and Cb % 64 == 0) or (Cb in (1, 3) and Cs % 32 == 0))


def _planned(planner, query, p):
    if query.startswith("stats"):
        arith = {"stats_bf16x3": BF16X3, "stats_f16": F16_2, "stats_f32": F32}[query]
        return planner.stats(p["family"], arith, p["B"], p["S"], p["S"], p["Cbig"], p["Csmall"], p["stride"]).stat_floats
    if query == "affine":
        return planner.affine(p["family"], p["precision"], p["B"], p["S"], p["S"], p["Cbig"], p["Csmall"], p["stride"]).affine_ok
    return planner.wgrad(BF16X3 if query == "wgrad_bf16x3" else F32, *G.call_args(query, p)).query_floats


@pytest.mark.parametrize("query", list(G.QUERIES))
def test_query_returns_what_the_parent_library_returned(planner, golden, query):
    assert golden["axes"] == G.AXES, "the golden file was recorded over another grid"
    rec = golden["queries"][query]
    assert tuple(rec["axes"]) == G.QUERIES[query][1]
    pts = list(G.points(query))
    codes = G.unrle(rec["rle"])
    assert len(codes) == len(pts)
    want = [G.decode(query, p, c) for p, c in zip(pts, codes)]
    checked, bad = 0, []
    for p, w in zip(pts, want):
        if query == "wgrad_f32" and _narrow_wgrad(p):
            continue
        checked += 1
        got = _planned(planner, query, p)
        if got != w:
            bad.append((p, got, w))
    assert not bad, f"{query}: {len(bad)} of {checked} differ, first {bad[:3]}"
    assert checked > 0.9 * len(pts)


def expected_launch(c, pl):
    """(substrings of the demangled kernel name, grid in workgroups or None, workgroup size) of a branch case's plan"""
    tf = ("false", "true")
    if c["kind"] == "wgrad":
        if pl.route == W_ROWS:
            total = (c["Csmall"] // 128) * (c["Cbig"] // pl.kind) * 5 * pl.nsplit
            name = f"vp::wgrad5f_kernel<{pl.kind}, " if c["arith"] == F32 else f"vp::wgrad5_kernel<{pl.kind}, {int(c['arith'] != BF16X3)}>"
            return [name], (8 * ceil_div(total, 8), 1, 1), 512
        prob = f"vp::ProbW16T<{tf[c['ks'] == 5]}, {int(c['arith'] == F16_2)}, {tf[pl.route == W_WIDE and pl.kind != 4]}>"
        tile = f", {pl.bm}, {pl.bn}, 2, 2, {pl.bk}, {tf[pl.fast]}, false>"
        return ["vp::igemm16_kernel<" + prob + tile], (ceil_div(c["Csmall"], pl.bm), ceil_div(pl.N, pl.bn), pl.gz), 256
    if pl.route == HALO:
        return ["vp::halo_conv_kernel<"], None, 256
    grid = (ceil_div(pl.M, pl.bm), ceil_div(pl.N, pl.bn), pl.gz)
    if pl.route == PIPELINED:
        return [f"vp::igemm16p_kernel<vp::{('PF16', 'PT16')[c['family']]}, {pl.bm}, {pl.bn}, ", f", true, {tf[pl.m16]}>"], grid, 512 if pl.bm == 256 and pl.bn >= 128 else 256
    prob = f"vp::Prob{'FT'[c['family']]}16T<true, {c['arith']}>"
    if c["kind"] == "affine":
        prob = f"vp::ProbAff<{prob} >"
    wm, wn = (4, 1) if pl.bn == 32 else (2, 2)
    return [f"vp::igemm16_kernel<{prob}, {pl.bm}, {pl.bn}, {wm}, {wn}, {pl.bk}, {tf[pl.fast]}, {tf[pl.m16]}>"], grid, 256


def test_recorded_launches_match_the_plan(planner, golden):
    """per branch case (tests/test_gpu_launch_plan_branches.py) what the parent's library launched on an MI355X, from a kernel trace:
    demangled kernel name, grid, workgroup size and whether a memset precedes it -- against what the planner's fields say"""
    from tests import test_gpu_launch_plan_branches as T
    launches = {r["case"]: r for r in golden["launches"]}
    assert set(launches) == set(T.BRANCHES), "record the launches again (tools/gen_golden_launch_plans.py --launches) when the case list changes"
    for name, c in T.BRANCHES.items():
        rec, pl = launches[name], T.plan_of(planner, c)
        parts, grid, wg = expected_launch(c, pl)
        assert all(p in rec["kernel"] for p in parts), (name, rec["kernel"], parts)
        assert grid is None or tuple(rec["grid"]) == grid, (name, rec["grid"], grid)
        assert rec["workgroup"] == wg, (name, rec["workgroup"], wg)
        if c["kind"] != "wgrad" and pl.route != HALO:
            assert bool(rec["memset"]) == bool(pl.zero_fill), (name, rec["memset"], pl.zero_fill)


# ---- 2. invariants over the whole sweep ---------------------------------------------------------------------------------------------
def _sweep():
    return itertools.product(G.BATCH, G.SIDE, G.CHAN, G.CHAN, G.STRIDE)


@pytest.mark.parametrize("arith", [BF16X3, F16_2, F16_3, F32], ids=["bf16x3", "f16x2", "f16x3", "f32"])
@pytest.mark.parametrize("family", [0, 1], ids=["gather", "scatter"])
def test_conv_plan_invariants(planner, family, arith):
    n = 0
    for B, S, Cb, Cs, stride in _sweep():
        if arith != F32 and (Cb if family == 0 else Cs) % 8:
            continue          # the 16-bit entry points take contracted channel counts that are multiples of 8
        for epi in ((EPI_NONE, EPI_STAT, EPI_AFFINE) if arith in (BF16X3, F32) else (EPI_NONE, EPI_STAT)):
            pl = planner.conv(family, arith, B, S, S, Cb, Cs, stride, epi=epi)
            ctx = (family, arith, epi, B, S, Cb, Cs, stride, dict(pl))
            n += 1
            assert (pl.nsplit == 2) == bool(pl.zero_fill) and pl.nsplit in (1, 2), ctx
            if pl.nsplit == 2:
                assert not pl.stat_ok and not pl.affine_ok, ctx
            assert pl.stat_ok == 0 or epi == EPI_STAT, ctx
            assert pl.affine_ok == 0 or epi == EPI_AFFINE, ctx
            if pl.route == HALO:
                assert arith == BF16X3 and epi != EPI_AFFINE and not pl.stat_ok, ctx
                continue
            assert pl.M == B * S * S and pl.N == (Cs if family == 0 else Cb), ctx
            assert pl.gz == pl.nsplit * (stride * stride if family else 1), ctx
            if pl.route == PIPELINED:
                assert arith == BF16X3 and epi != EPI_AFFINE, ctx
                assert PCFG[pl.kind] == (pl.bm, pl.bn) and pl.bm <= pl.M and pl.bn <= pl.N, ctx
                assert bool(pl.m16) == (pl.kind == 3) and not (pl.m16 and epi == EPI_STAT), ctx
                assert pl.pair_phases == 0, ctx
            elif pl.route == LEGACY:      # (its tile fields are what the fast path would have run: unused)
                assert arith == F32 and not pl.affine_ok, ctx
            else:
                assert (pl.bm, pl.bn) in ((128, 128), (128, 64), (64, 64), (256, 32), (128, 32)), ctx
                assert pl.bn != 32 or (pl.bk == 32 and arith != F32), ctx
                if pl.m16:      # only on the tiles and problem types that instantiate it
                    assert arith == BF16X3 and epi != EPI_AFFINE and pl.bk == 64 and pl.fast and pl.bm == 128 and pl.bn in (128, 64), ctx
                    assert pl.bn == 128 or (family == 1 and pl.M >= 65536), ctx
                if pl.route == STAGED and arith == F32:
                    assert pl.fast and pl.bn != 32, ctx
            assert pl.xcd_map == int(ceil_div(pl.M, pl.bm) % 8 == 0 and ceil_div(pl.N, pl.bn) >= 2), ctx
            if pl.nsplit == 2:
                assert pl.k_per_split % 64 == 0 and pl.k_per_split < pl.K <= 2 * pl.k_per_split, ctx
            else:
                assert pl.k_per_split == pl.K, ctx
            if pl.stat_ok:
                assert pl.stat_floats == 3 * pl.N * ceil_div(pl.M, pl.bm) * pl.gz and pl.stat_tiles_m == ceil_div(pl.M, pl.bm), ctx
                assert pl.stat_R == pl.M * (stride * stride if family else 1), ctx
            else:
                assert pl.stat_floats == 0, ctx
            if pl.affine_ok:
                assert pl.bn != 32 and pl.nsplit == 1 and pl.route == STAGED and pl.bk == 64 and pl.fast and not pl.m16, ctx
    assert n > 10000


@pytest.mark.parametrize("arith", [BF16X3, F16_2, F32], ids=["bf16x3", "f16x2", "f32"])
def test_wgrad_plan_invariants(planner, arith):
    n = 0
    for B, S, Cb, Cs, stride in _sweep():
        for ks in G.KS:
            if arith != F32 and (Cb % 8 or Cs % 8):
                continue
            Hb = G.big_side(S, ks, stride)
            q = planner.wgrad(arith, B, S, S, Hb, Hb, Cb, Cs, ks, stride)
            assert q.need_floats <= q.query_floats, (arith, B, S, Cb, Cs, ks, stride, dict(q))
            for cus in (0, 1, 96, 128, 160, 256, 1000):
                for ws in ((-1, 4 * q.query_floats, 4 * q.need_floats) if cus == 0 else (-1,)):
                    w = planner.wgrad(arith, B, S, S, Hb, Hb, Cb, Cs, ks, stride, max_cus=cus, ws_bytes=ws)
                    ctx = (arith, B, S, Cb, Cs, ks, stride, cus, ws, dict(w))
                    n += 1
                    assert w.query_floats == q.query_floats, ctx
                    assert w.slab_floats <= w.query_floats and w.slab_floats <= max(ws, 4 * q.query_floats) // 4, ctx
                    assert w.slabs * ks * ks * Cs * Cb == w.slab_floats, ctx
                    assert w.nsplit >= 1 and w.k_per_split % 32 == 0 and w.nsplit * w.k_per_split >= B * S * S, ctx
                    if w.route == W_ROWS:
                        assert (w.nsplit - 1) * w.k_per_split < B * S * S, ctx          # no empty split (the other kernels skip an empty one)
                        assert w.kind in (64, 128) and ks == 5 and stride == 2 and Cs % 128 == 0, ctx
                    elif w.route == W_WIDE:
                        assert arith == BF16X3 and (w.bm, w.bn) == {1: (64, 64), 2: (128, 128), 3: (64, 128), 4: (64, 128)}[w.kind], ctx
                        assert Cs % w.bm == 0 and w.N % w.bn == 0 and w.bk == 32 and w.fast, ctx
                    elif w.route == W_MAIN:
                        assert arith != F32 and w.gz == ks * ks * w.nsplit and w.N == Cb, ctx
                        assert w.bk == 32 or (arith == F16_2 and w.bn != 32), ctx
                    else:
                        assert arith == F32, ctx
    assert n > 10000


# ---- 3. the switches, by value --------------------------------------------------------------------------------
def test_switches_change_the_routes_they_name(planner):
    P = planner
    # VP_IGEMM16P: 0 pipelined kernel off; 2 = only the 256x256 rule
    big, small = (0, BF16X3, 2, 128, 128, 32, 512, 1), (0, BF16X3, 2, 8, 8, 32, 128, 1)
    assert P.conv(*big).kind == 6 and P.conv(*small).kind == 7
    assert P.conv(*big, sw=dict(igemm16p_mode=0)).route == STAGED and P.conv(*small, sw=dict(igemm16p_mode=0)).route == STAGED
    assert P.conv(*big, sw=dict(igemm16p_mode=2)).kind == 6 and P.conv(*small, sw=dict(igemm16p_mode=2)).route == STAGED
    # VP_IGEMM16P_M16: the 256x128 tile on the 16x16x32 form, one gather shape
    pm16 = (0, BF16X3, 1, 128, 128, 128, 256, 1)
    assert P.conv(*pm16).kind == 3 and P.conv(*pm16).m16 == 1
    off = P.conv(*pm16, sw=dict(igemm16p_m16=0))
    assert off.route == STAGED and off.m16 == 0
    assert P.conv(*pm16, sw=dict(igemm16_m16=0)).kind == 3          # (the staged kernels' switch leaves it alone)
    # VP_IGEMM16_M16: the 16x16x32 form of the staged kernels
    sm16 = (0, BF16X3, 6, 64, 64, 64, 136, 1)
    on, no = P.conv(*sm16), P.conv(*sm16, sw=dict(igemm16_m16=0))
    assert on.route == STAGED and on.m16 == 1 and no.m16 == 0 and (no.route, no.bm, no.bn, no.bk, no.fast) == (on.route, on.bm, on.bn, on.bk, on.fast)
    assert P.conv(*sm16, sw=dict(igemm16p_m16=0)).m16 == 1
    # VP_F32_FAST: the fp32 fast path, its statistics and its affine epilogue
    f = (0, F32, 32, 16, 16, 64, 128, 2)
    assert P.conv(*f).route == STAGED and P.conv(*f, sw=dict(f32_fast=0)).route == LEGACY
    assert P.stats(0, F32, 32, 16, 16, 64, 128, 2).stat_floats > 0 and P.stats(0, F32, 32, 16, 16, 64, 128, 2, sw=dict(f32_fast=0)).stat_floats == 0
    assert P.affine(0, 1, 32, 16, 16, 64, 128, 2).affine_ok == 1 and P.affine(0, 1, 32, 16, 16, 64, 128, 2, sw=dict(f32_fast=0)).affine_ok == 0
    assert P.affine(0, 0, 32, 16, 16, 64, 128, 2, sw=dict(f32_fast=0)).affine_ok == 1
    # VP_WGRAD5 / VP_WGRAD5F: rows of taps, split-operand / fp32; each leaves the other arithmetic alone
    w = (32, 16, 16, 32, 32, 128, 128, 5, 2)
    assert P.wgrad(BF16X3, *w).route == W_ROWS and P.wgrad(BF16X3, *w, sw=dict(wgrad5=0)).route == W_MAIN
    assert P.wgrad(F32, *w).route == W_ROWS and P.wgrad(F32, *w, sw=dict(wgrad5f=0)).route == W_LEGACY
    assert P.wgrad(F32, *w, sw=dict(wgrad5=0)).route == W_ROWS and P.wgrad(BF16X3, *w, sw=dict(wgrad5f=0)).route == W_ROWS
    # VP_WGRAD5_BLOCKS overrides the caller's work-item count
    assert P.wgrad(BF16X3, *w, max_cus=128, sw=dict(wgrad5_blocks=40)).nsplit == 8 and P.wgrad(BF16X3, *w, max_cus=128).nsplit == 24
    # VP_WGRAD_PAIR16: tap pairs at 16 taps
    w4 = (4, 16, 16, 32, 32, 64, 128, 4, 2)
    assert P.wgrad(BF16X3, *w4).route == W_WIDE and P.wgrad(BF16X3, *w4).kind == 2
    assert P.wgrad(BF16X3, *w4, sw=dict(wgrad_pair16=0)).route == W_MAIN
    w3 = (4, 16, 16, 32, 32, 64, 128, 3, 2)
    assert P.wgrad(BF16X3, *w3, sw=dict(wgrad_pair16=0)).route == W_WIDE


# ---- 4. the GPU test's shapes take the branches they are listed for ---------------------------------------------------------------------
def test_branch_shapes_take_their_branch(planner):
    from tests import test_gpu_launch_plan_branches as T
    for name, case in {**T.BRANCHES, **T.VARIANTS}.items():
        got = T.plan_of(planner, case)
        for k, v in case["expect"].items():
            assert got[k] == v, f"{name}: {k} = {got[k]}, listed for {v} ({dict(got)})"
