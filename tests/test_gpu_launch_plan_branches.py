"""Every branch of the launch planner (vae_play_amd/csrc/launch_plan.h) once on the GPU: one C-ABI call per branch at the smallest
shape that takes it, outputs NaN-prefilled and guarded (tests/guarded.py), workspaces of exactly the queried size, results against
the fp64 direct sums of tests/conv_ref.py with the tolerances of tests/test_gpu_conv_direct_kxk.py (conv_ref.tau) and
tests/test_gpu_conv_affine.py; the statistics entries also compare mean and rstd with fp64 (the bounds of
tests/test_gpu_properties.py).

The shapes were found by brute force over the planner on a CPU, minimising M * N * K over B in {1 .. 128}, Hs = Ws in {4 .. 128},
channel counts that are multiples of 8 up to 256 (and 384, 512), stride 1 | 2.  `expect` names the plan fields that define the branch;
tests/test_launch_plan.py asserts on a CPU that each shape still takes it.  The rows of taps run at 8 images of 32 x 32 small
pixels, the smallest of the grid at which a budget of 128 work items splits the pixels less deeply than the whole chip."""
import hashlib

import pytest
import torch

from tests import conv_ref as R
from tests.guarded import Guards

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16X3, F16_2, F16_3, F32 = range(4)
LEGACY, HALO, PIPELINED, STAGED = range(4)
W_LEGACY, W_ROWS, W_WIDE, W_MAIN = range(4)
MODE = {BF16X3: "bf16x3", F16_2: "f16x2/2", F16_3: "f16x2/3", F32: "f32"}
GSCALE = 16.0     # power-of-two scale of the gradient operand of the two-product weight gradient (undone by out_scale)


def _conv(family, arith, B, S, Cbig, Csmall, stride, **expect):
    return dict(kind="conv", family=family, arith=arith, B=B, S=S, Cbig=Cbig, Csmall=Csmall, stride=stride, ks=5, expect=expect)


def _stats(family, arith, B, S, Cbig, Csmall, stride, **expect):
    return dict(_conv(family, arith, B, S, Cbig, Csmall, stride, stat_ok=1, **expect), kind="stats")


def _affine(family, arith, B, S, Cbig, Csmall, stride, **expect):
    return dict(_conv(family, arith, B, S, Cbig, Csmall, stride, affine_ok=1, route=STAGED, bk=64, fast=1, **expect), kind="affine")


def _wgrad(arith, B, S, Cbig, Csmall, stride, ks, max_cus=0, **expect):
    return dict(kind="wgrad", arith=arith, B=B, S=S, Cbig=Cbig, Csmall=Csmall, stride=stride, ks=ks, max_cus=max_cus, expect=expect)


BRANCHES = {
    # ---- gather (family 0) and scatter (family 1), split bf16 ----
    "halo_gather_kind1": _conv(0, BF16X3, 1, 16, 32, 8, 1, route=HALO, kind=1),
    "halo_gather_kind2": _conv(0, BF16X3, 1, 16, 32, 64, 2, route=HALO, kind=2),
    "halo_gather_kind3": _conv(0, BF16X3, 1, 16, 8, 8, 2, route=HALO, kind=3),
    "halo_scatter_kind1": _conv(1, BF16X3, 1, 16, 8, 8, 1, route=HALO, kind=1),
    "pipelined_256x256_gather": _conv(0, BF16X3, 2, 128, 32, 512, 1, route=PIPELINED, kind=6, bm=256, bn=256),
    "pipelined_256x256_scatter": _conv(1, BF16X3, 1, 128, 256, 32, 2, route=PIPELINED, kind=6, gz=4),
    "pipelined_128x64_gather": _conv(0, BF16X3, 2, 8, 32, 128, 1, route=PIPELINED, kind=7, bm=128, bn=64),
    "pipelined_128x64_scatter": _conv(1, BF16X3, 2, 8, 128, 32, 2, route=PIPELINED, kind=7, gz=4),
    "pipelined_256x128_m16_gather": _conv(0, BF16X3, 1, 128, 128, 256, 1, route=PIPELINED, kind=3, bm=256, bn=128, m16=1),
    "staged_128x128_m16_gather": _conv(0, BF16X3, 6, 64, 64, 136, 1, route=STAGED, bm=128, bn=128, bk=64, fast=1, m16=1),
    "staged_128x128_m16_scatter": _conv(1, BF16X3, 6, 64, 136, 64, 1, route=STAGED, bm=128, bn=128, bk=64, fast=1, m16=1),
    "staged_128x64_m16_scatter_from_65536_rows": _conv(1, BF16X3, 4, 128, 64, 64, 1, route=STAGED, bm=128, bn=64, m16=1, M=65536),
    "staged_128x128_with_tails_gather": _conv(0, BF16X3, 6, 64, 8, 136, 1, route=STAGED, bm=128, bn=128, bk=64, fast=0, m16=0),
    "staged_128x64_gather": _conv(0, BF16X3, 6, 64, 64, 72, 1, route=STAGED, bm=128, bn=64, bk=64, fast=1, m16=0),
    "staged_64x64_fast64_gather": _conv(0, BF16X3, 1, 4, 64, 8, 1, route=STAGED, bm=64, bn=64, bk=64, fast=1, nsplit=1),
    "staged_64x64_fast32_c32_scatter": _conv(1, BF16X3, 1, 4, 8, 32, 1, route=STAGED, bm=64, bn=64, bk=32, fast=1),
    "staged_64x64_c40_chunks_with_tails_gather": _conv(0, BF16X3, 1, 4, 40, 8, 1, route=STAGED, bm=64, bn=64, bk=64, fast=0),
    "staged_64x64_with_tails_gather": _conv(0, BF16X3, 1, 4, 8, 8, 1, route=STAGED, bm=64, bn=64, bk=64, fast=0),
    "staged_256x32_gather": _conv(0, BF16X3, 6, 128, 32, 8, 2, route=STAGED, bm=256, bn=32, bk=32, fast=1),
    "staged_128x32_scatter": _conv(1, BF16X3, 2, 8, 8, 32, 1, route=STAGED, bm=128, bn=32, bk=32, fast=1),
    "staged_128x32_with_tails_scatter": _conv(1, BF16X3, 2, 8, 8, 8, 1, route=STAGED, bm=128, bn=32, bk=32, fast=0),
    "splitk_gather": _conv(0, BF16X3, 1, 4, 192, 8, 1, route=STAGED, nsplit=2, zero_fill=1, gz=2),
    "splitk_scatter": _conv(1, BF16X3, 1, 4, 8, 256, 1, route=STAGED, nsplit=2, zero_fill=1, gz=2),
    "phase_pairs_on": _conv(1, BF16X3, 1, 4, 8, 8, 2, route=STAGED, pair_phases=1, gz=4),
    "phase_pairs_off": _conv(1, BF16X3, 8, 48, 8, 8, 2, route=STAGED, pair_phases=0, gz=4),
    "f16_two_products_gather": _conv(0, F16_2, 1, 4, 64, 8, 1, route=STAGED, bk=64, fast=1),
    "f16_three_products_scatter": _conv(1, F16_3, 1, 4, 8, 64, 2, route=STAGED, bk=64, fast=1, gz=4),
    # ---- the statistics epilogue ----
    "stats_pipelined_gather": _stats(0, BF16X3, 2, 8, 32, 128, 1, route=PIPELINED, kind=7),
    "stats_pipelined_scatter": _stats(1, BF16X3, 2, 8, 128, 32, 2, route=PIPELINED, kind=7, gz=4),
    "stats_staged_gather": _stats(0, BF16X3, 1, 4, 8, 8, 1, route=STAGED, bm=64, bn=64),
    "stats_staged_m16_scatter": _stats(1, BF16X3, 6, 64, 136, 64, 1, route=STAGED, bm=128, bn=128, m16=1),
    "stats_f16_gather": _stats(0, F16_3, 1, 4, 8, 8, 1, route=STAGED),
    "stats_f32_scatter": _stats(1, F32, 1, 4, 64, 16, 1, route=STAGED, bk=32),
    # ---- the fp32 fast path ----
    "f32_k64_gather": _conv(0, F32, 1, 4, 32, 64, 1, route=STAGED, bk=64, fast=1, nsplit=1),
    "f32_k32_gather": _conv(0, F32, 1, 4, 16, 64, 1, route=STAGED, bk=32, fast=1),
    "f32_k32_scatter": _conv(1, F32, 1, 4, 64, 16, 1, route=STAGED, bk=32, fast=1),
    "f32_splitk_gather": _conv(0, F32, 1, 4, 96, 64, 1, route=STAGED, nsplit=2, zero_fill=1),
    "f32_splitk_scatter": _conv(1, F32, 1, 4, 64, 128, 1, route=STAGED, nsplit=2, zero_fill=1),
    # ---- the affine epilogue ----
    "affine_bf16x3_gather": _affine(0, BF16X3, 1, 4, 64, 64, 1),
    "affine_bf16x3_scatter": _affine(1, BF16X3, 1, 4, 64, 64, 2, gz=4, pair_phases=1),
    "affine_f32_gather": _affine(0, F32, 1, 4, 32, 64, 1),
    "affine_f32_scatter": _affine(1, F32, 1, 4, 64, 32, 2, gz=4, pair_phases=1),
    # ---- weight gradient ----
    "wgrad_rows_bn64_whole_chip": _wgrad(BF16X3, 8, 32, 64, 128, 2, 5, 0, route=W_ROWS, kind=64, nsplit=43, slabs=86),
    "wgrad_rows_bn64_128_items": _wgrad(BF16X3, 8, 32, 64, 128, 2, 5, 128, route=W_ROWS, kind=64, nsplit=24, slabs=48),
    "wgrad_rows_bn128_whole_chip": _wgrad(BF16X3, 8, 32, 128, 128, 2, 5, 0, route=W_ROWS, kind=128, nsplit=43, slabs=43),
    "wgrad_rows_bn128_128_items": _wgrad(BF16X3, 8, 32, 128, 128, 2, 5, 128, route=W_ROWS, kind=128, nsplit=24, slabs=24),
    "wgrad_rows_f16_bn128": _wgrad(F16_2, 1, 8, 128, 128, 2, 5, 0, route=W_ROWS, kind=128),
    "wgrad_rows_f32_bn64": _wgrad(F32, 1, 8, 64, 128, 2, 5, 0, route=W_ROWS, kind=64),
    "wgrad_wide_kind1": _wgrad(BF16X3, 1, 4, 32, 64, 1, 3, route=W_WIDE, kind=1, bm=64, bn=64),
    "wgrad_wide_kind2": _wgrad(BF16X3, 1, 4, 64, 128, 1, 3, route=W_WIDE, kind=2, bm=128, bn=128),
    "wgrad_wide_kind3": _wgrad(BF16X3, 1, 4, 64, 64, 1, 3, route=W_WIDE, kind=3, bm=64, bn=128),
    "wgrad_wide_kind4": _wgrad(BF16X3, 1, 4, 128, 64, 1, 3, route=W_WIDE, kind=4, bm=64, bn=128),
    "wgrad_main_fast": _wgrad(BF16X3, 1, 4, 192, 64, 1, 3, route=W_MAIN, bk=32, fast=1),
    "wgrad_main_with_tails": _wgrad(BF16X3, 1, 4, 8, 8, 1, 3, route=W_MAIN, bk=32, fast=0),
    "wgrad_main_f16_k64": _wgrad(F16_2, 1, 4, 64, 64, 1, 3, route=W_MAIN, bk=64, fast=1),
}

# What the descriptor fillers of csrc/conv_exec.h fill beyond BRANCHES: the epilogue fields (bias, sigmoid, out_scale, running
# statistics, the affine outputs), the generic-geometry descriptors (ks = 1, 3 and 4 x 4 stride 2) in the three 16-bit arithmetics,
# the plain 5 x 5 stride-1 weight gradient and the fp32 entries outside the fast path.  Smallest shapes: 1 image, 4 x 4 small side.
# Extra keys: ks, bias, act, out_scale, running (non-null running statistics), outputs ("f32" | "split" | "both", affine).
def _with(case, **extra):
    return dict(case, **extra)


_TAG = {BF16X3: "bf16x3", F16_2: "f16_two_products", F16_3: "f16_three_products"}
VARIANTS = {
    "gather_bias_sigmoid": _with(_conv(0, BF16X3, 1, 4, 64, 8, 1, route=STAGED, nsplit=1), bias=1, act=4),
    **{f"k{ks}_{('gather', 'scatter')[fam]}_{_TAG[ar]}": _with(_conv(fam, ar, 1, 4, 16, 8, st, route=STAGED, nsplit=1), ks=ks)
       for ks, st in ((1, 1), (3, 1), (4, 2)) for fam in (0, 1) for ar in (BF16X3, F16_2, F16_3)},
    "scatter_bias_plain5": _with(_conv(1, BF16X3, 1, 4, 8, 8, 1, route=STAGED), bias=1),
    "scatter_bias_k4_stride2": _with(_conv(1, BF16X3, 1, 4, 8, 8, 2, route=STAGED, gz=4), ks=4, bias=1),
    "f16_out_scale_gather": _with(_conv(0, F16_2, 1, 4, 64, 8, 1, route=STAGED), out_scale=1.0 / 16),
    "stats_running_f16_two_products_gather": _with(_stats(0, F16_2, 1, 4, 8, 8, 1, route=STAGED), running=1),
    "stats_running_f16_three_products_scatter": _with(_stats(1, F16_3, 1, 4, 8, 8, 1, route=STAGED), running=1),
    "stats_running_f32_gather": _with(_stats(0, F32, 1, 4, 16, 64, 1, route=STAGED), running=1),
    "affine_split_planes_only": _with(_affine(0, BF16X3, 1, 4, 64, 64, 1), outputs="split"),
    "affine_both_outputs": _with(_affine(1, BF16X3, 1, 4, 64, 64, 2, gz=4, pair_phases=1), outputs="both"),
    "affine_act_none": _with(_affine(0, F32, 1, 4, 32, 64, 1), act=0),
    "wgrad_plain5_stride1_bf16x3": _wgrad(BF16X3, 1, 4, 64, 64, 1, 5, route=W_WIDE, kind=3),
    "wgrad_plain5_stride1_f16": _wgrad(F16_2, 1, 4, 64, 64, 1, 5, route=W_MAIN),
    "f32_legacy_gather": _conv(0, F32, 1, 4, 8, 8, 1, route=LEGACY),
    "f32_scatter_bias_k4_stride2": _with(_conv(1, F32, 1, 4, 8, 8, 2), ks=4, bias=1),     # always igemm.h: no plan
}


def plan_of(planner, c):
    """the plan of a case, from tests/test_launch_plan.py's Planner"""
    S = c["S"]
    Hb = S * c["stride"]
    if c["kind"] == "wgrad":
        return planner.wgrad(c["arith"], c["B"], S, S, Hb, Hb, c["Cbig"], c["Csmall"], c["ks"], c["stride"], max_cus=c["max_cus"])
    epi = {"conv": 0, "stats": 1, "affine": 2}[c["kind"]]
    return planner.conv(c["family"], c["arith"], c["B"], S, S, c["Cbig"], c["Csmall"], c["stride"], ks=c["ks"], Hb=Hb, Wb=Hb,
                        has_bias=c.get("bias", 0), act=c.get("act", 0) if c["kind"] == "conv" else 0, epi=epi)


def _nhwc(B, C, H, W, gen):
    return torch.randn(B, H, W, C, device=DEV, generator=gen).permute(0, 3, 1, 2)


def _operands(c, name):
    """x (big side), y (small side), w [Cs][Cb][ks][ks] of a case, seeded by its name"""
    gen = torch.Generator(device=DEV).manual_seed(sum(map(ord, name)))
    S, st = c["S"], c["stride"]
    Hb = S * st
    x, y = _nhwc(c["B"], c["Cbig"], Hb, Hb, gen), _nhwc(c["B"], c["Csmall"], S, S, gen)
    w = torch.randn(c["Csmall"], c["Cbig"], c["ks"], c["ks"], device=DEV, generator=gen) * 0.05
    return x, y, w, gen


def _packed(w, arith, family):
    """the family's packed weight: fp32, or split planes of the arithmetic's format"""
    from vae_play_amd import ops
    if arith == F32:
        return ops.pack_w(w, family == 0, family == 1)[family]
    if arith == BF16X3:
        return ops.pack_w_split(w, family == 0, family == 1)[family]
    if w.shape[2] != 5:      # no k x k packer writes fp16 pairs: the fp32 layout (a permutation), then the element-wise split
        return ops.split_f32(ops.pack_w(w, family == 0, family == 1)[family], ops.SPLIT_F16)
    return ops.pack_w5_split(w, family == 0, family == 1, ops.SPLIT_F16)[family]


def _act(t, arith, scale=1.0):
    from vae_play_amd import ops
    if arith == F32:
        return t.contiguous(memory_format=torch.channels_last)
    return ops.split_f32(t, ops.SPLIT_BF16 if arith == BF16X3 else ops.SPLIT_F16, scale)


def run_case(name, c):
    """one C-ABI call on guarded buffers -> (outputs by name, operands); every output is checked for sentinels and NaN"""
    from vae_play_amd import _lib, ops
    lib = _lib.load()
    x, y, w, gen = _operands(c, name)
    B, S, st, Cb, Cs, ks, ar = c["B"], c["S"], c["stride"], c["Cbig"], c["Csmall"], c["ks"], c["arith"]
    Hb = S * st
    g = Guards(DEV)
    P, PV, stream = ops._p, ops._pv, ops._stream()
    ptr = P if ar == F32 else PV
    suffix = {BF16X3: "bf16x3", F16_2: "f16", F16_3: "f16", F32: "f32"}[ar]
    products = () if ar in (BF16X3, F32) else ((2,) if ar == F16_2 else (3,))
    outs = {}
    if c["kind"] == "wgrad":
        dw = g.out("dw", Cs, Cb, ks, ks)
        query = lib.vp_conv_wgrad_workspace_bytes if ar == F32 else lib.vp_conv_wgrad_bf16x3_workspace_bytes
        ws, nbytes = g.ws("ws", query(B, S, S, Hb, Hb, Cb, Cs, ks, st))
        geom = (B, S, S, Hb, Hb, Cb, Cs, ks, st)
        geom5 = (B, S, S, Cb, Cs, st)
        if ar == F32:
            xa, ya = _act(x, ar), _act(y, ar)
            if c["max_cus"] or ks == 5:
                _lib.call("vp_conv5_wgrad_f32_cus", P(xa), P(ya), P(dw), *geom5, c["max_cus"], P(ws), nbytes, stream)
            else:
                _lib.call("vp_conv_wgrad_f32", P(xa), P(ya), P(dw), *geom, P(ws), nbytes, stream)
        elif ar == BF16X3:
            xa, ya = _act(x, ar), _act(y, ar)
            if ks == 5 and st == 2:
                _lib.call("vp_conv5_wgrad_bf16x3_cus", PV(xa), PV(ya), P(dw), *geom5, c["max_cus"], P(ws), nbytes, stream)
            else:
                _lib.call("vp_conv_wgrad_bf16x3", PV(xa), PV(ya), P(dw), *geom, P(ws), nbytes, stream)
        else:      # two products: the gradient planes scaled by GSCALE, x keeps its hi plane only
            xa, ya = _act(x, ar), ops.split_f32(y, ops.SPLIT_F16, GSCALE)
            _lib.call("vp_conv_wgrad_f16x2", PV(xa), PV(ya), P(dw), *geom, 1.0 / GSCALE, P(ws), nbytes, stream)
        outs["dw"] = dw
    else:
        fam = c["family"]
        a, Cout, Ho = (x, Cs, S) if fam == 0 else (y, Cb, Hb)
        out = g.out("out", B, Ho, Ho, Cout).permute(0, 3, 1, 2)
        out_scale = c.get("out_scale", 1.0)
        ain, wp = _act(a, ar, 1.0 / out_scale), _packed(w, ar, fam)
        which = ("gather", "scatter")[fam]
        chans = (Cb, Cs) if fam == 0 else (Cs, Cb)
        bias = torch.randn(Cout, device=DEV, generator=gen) * 0.1 if c.get("bias") else None
        if bias is not None:
            outs["bias"] = bias
        if c["kind"] == "conv":
            scale = () if ar in (BF16X3, F32) else (out_scale,)
            if fam == 0:
                bias_act, entry = (P(bias),), f"vp_conv_gather_{suffix}"
            else:
                bias_act, entry = ((P(bias),), f"vp_conv_scatter_bias_{suffix}") if bias is not None else ((), f"vp_conv_scatter_{suffix}")
            _lib.call(entry, ptr(ain), ptr(wp), *bias_act, P(out), B, S, S, Hb, Hb, *chans, ks, st,
                      *((c.get("act", 0),) if fam == 0 else ()), *products, *scale, stream)
        elif c["kind"] == "stats":
            query = {"bf16x3": lib.vp_conv5_stats_workspace_bytes, "f16": lib.vp_conv5_stats_f16_workspace_bytes,
                     "f32": lib.vp_conv5_stats_f32_workspace_bytes}[suffix]
            ws, nbytes = g.ws("ws", query(fam, B, S, S, Cb, Cs, st))
            assert nbytes > 0, "the planner lists this shape as able to emit statistics"
            mean, rstd = g.out("mean", Cout), g.out("rstd", Cout)
            rm = rv = None
            if c.get("running"):
                outs["running_mean0"] = torch.randn(Cout, device=DEV, generator=gen)
                outs["running_var0"] = torch.rand(Cout, device=DEV, generator=gen) + 0.5
                rm, rv = g.state("running_mean", outs["running_mean0"]), g.state("running_var", outs["running_var0"])
                outs["running_mean"], outs["running_var"] = rm, rv
            _lib.call(f"vp_conv5_{which}_stats_{suffix}", ptr(ain), ptr(wp), P(out), B, S, S, *chans, st, *products, 1e-5, 0.9, P(mean), P(rstd),
                      P(rm), P(rv), P(ws), nbytes, stream)
            outs["mean"], outs["rstd"] = mean, rstd
        else:
            assert lib.vp_conv5_affine_supported(fam, 1 if ar == F32 else 0, B, S, S, Cb, Cs, st) == 1
            scale = torch.empty(Cout, device=DEV).uniform_(0.5, 1.5, generator=gen)
            scale[1::3] *= -1.0
            shift = torch.randn(Cout, device=DEV, generator=gen) * 0.2
            wanted = c.get("outputs", "f32")
            if wanted != "f32":
                outs["planes"] = g.planes("planes", out.numel())
            if wanted == "split":
                g.items = [it for it in g.items if it[0] != "out"]      # the fp32 output is not requested: nothing to check
                out = None
            _lib.call(f"vp_conv5_{which}_affine_{suffix}", ptr(ain), ptr(wp), P(scale), P(shift), P(out), PV(outs.get("planes")), B, S, S, *chans,
                      st, c.get("act", ops.ACT_RELU), stream)
            outs["scale"], outs["shift"] = scale, shift
        if out is not None:
            outs["out"] = out
    g.check()
    return outs, (x, y, w)


def _within(label, got, r, A, K, mode):
    ratio, i, err = R.worst_scaled(got, r, A, R.tau(K, mode).to(r.device))
    print(f"{label}: worst err / tau = {ratio:.3f}")
    assert ratio <= 1.0, f"{label}: |out - r| = {err:.2e} * A at flat sample {i} exceeds tau(K = {int(K.flatten()[i])}, {mode})"


@pytest.mark.parametrize("name", list(BRANCHES))
def test_branch_against_fp64_direct_sums(name):
    c = BRANCHES[name]
    outs, (x, y, w) = run_case(name, c)
    mode, st, ks = MODE[c["arith"]], c["stride"], c["ks"]
    if c["kind"] == "wgrad":
        cs, cb = R.tile_channels(c["Csmall"]), R.tile_channels(c["Cbig"])
        _within(name, outs["dw"][cs][:, cb], *R.wgrad_ref(x, y, cs, cb, ks, st, terms=True), mode)
        return
    fam, S = c["family"], c["S"]
    out = outs["out"]
    pts = R.gather_points(c["B"], S, 3) if fam == 0 else R.scatter_points(c["B"], S * st, 3)
    r, A, K = R.gather_ref(x, w, pts, st, terms=True) if fam == 0 else R.scatter_ref(y, w, pts, st, terms=True)
    got = R.take(out, pts)
    if c["kind"] == "affine":      # the bound of tests/test_gpu_conv_affine.py
        s64, t64 = outs["scale"].double()[None, :], outs["shift"].double()[None, :]
        ref = torch.relu(r * s64 + t64)
        bound = s64.abs() * R.tau(K, mode).to(r.device) * A + R.SAFETY * 2 * 2.0 ** -24 * ((r * s64).abs() + t64.abs())
        worst = ((got - ref).abs() / bound).max().item()
        print(f"{name}: worst |v - ref| / bound = {worst:.3f}")
        assert worst <= 1.0
        return
    _within(name, got, r, A, K, mode)
    if c["kind"] == "stats":       # the bounds of tests/test_gpu_properties.py, against fp64 moments of the launch's own output
        xd = out.double()
        m64, v64 = xd.mean(dim=(0, 2, 3)), xd.var(dim=(0, 2, 3), unbiased=False)
        sig = v64.sqrt()
        em = ((outs["mean"].double() - m64).abs() / sig).max().item()
        er = ((outs["rstd"].double() - (v64 + 1e-5).rsqrt()).abs() * sig).max().item()
        print(f"{name}: mean {em:.2e}, rstd {er:.2e} (of 1e-5)")
        assert em <= 1e-5 and er <= 1e-5


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variant_against_fp64_direct_sums(name):
    """the references and bounds of the branch test; a bias is one more term (tests/test_gpu_conv_direct_kxk.py), the sigmoid is held to
    OP_RTOL like tests/test_gpu_parity.py's, the split planes and the running statistics as in tests/test_gpu_conv_affine.py and
    tests/test_gpu_properties.py"""
    from vae_play_amd import ops
    from tests.util import OP_RTOL, assert_close
    c = VARIANTS[name]
    outs, (x, y, w) = run_case(name, c)
    mode, st, ks = MODE[c["arith"]], c["stride"], c["ks"]
    if c["kind"] == "wgrad":
        cs, cb = R.tile_channels(c["Csmall"]), R.tile_channels(c["Cbig"])
        _within(name, outs["dw"][cs][:, cb], *R.wgrad_ref(x, y, cs, cb, ks, st, terms=True), mode)
        return
    fam, S = c["family"], c["S"]
    pts = R.gather_points(c["B"], S, 3) if fam == 0 else R.scatter_points(c["B"], S * st, 3)
    r, A, K = R.gather_ref(x, w, pts, st, terms=True) if fam == 0 else R.scatter_ref(y, w, pts, st, terms=True)
    if "bias" in outs:
        b64 = outs["bias"].double()
        r, A, K = r + b64, A + b64.abs(), K + 1
    if c["kind"] == "affine":
        s64, t64 = outs["scale"].double()[None, :], outs["shift"].double()[None, :]
        ref = r * s64 + t64
        ref = torch.relu(ref) if c.get("act", ops.ACT_RELU) == ops.ACT_RELU else ref
        bound = s64.abs() * R.tau(K, mode).to(r.device) * A + R.SAFETY * 2 * 2.0 ** -24 * ((r * s64).abs() + t64.abs())
        if "out" in outs:
            worst = ((R.take(outs["out"], pts) - ref).abs() / bound).max().item()
            print(f"{name}: worst |v - ref| / bound = {worst:.3f}")
            assert worst <= 1.0
        if "planes" in outs:      # hi + lo keep 16 significant bits (csrc/split.h): that plus 2^-16 |v|
            B, Ho, Cout = c["B"], S if fam == 0 else S * st, ref.shape[1]
            rec = R.take(ops.unsplit(outs["planes"]).view(B, Ho, Ho, Cout).permute(0, 3, 1, 2), pts)
            worst = ((rec - ref).abs() / (bound + 2.0 ** -16 * ref.abs())).max().item()
            print(f"{name}: planes, worst |hi + lo - ref| / bound = {worst:.3f}")
            assert worst <= 1.0
            if "out" in outs:
                assert torch.equal(outs["planes"], ops.split_f32(outs["out"].permute(0, 2, 3, 1).contiguous()).view(2, -1))
        return
    got = R.take(outs["out"], pts)
    if c.get("act") == ops.ACT_SIGMOID:
        print(f"{name}: sigmoid, rel err {assert_close(got, torch.sigmoid(r), OP_RTOL, name):.2e}")
        return
    _within(name, got, r, A, K, mode)
    if c["kind"] == "stats":
        out = outs["out"]
        xd = out.double()
        m64, v64 = xd.mean(dim=(0, 2, 3)), xd.var(dim=(0, 2, 3), unbiased=False)
        sig = v64.sqrt()
        assert ((outs["mean"].double() - m64).abs() / sig).max().item() <= 1e-5
        assert ((outs["rstd"].double() - (v64 + 1e-5).rsqrt()).abs() * sig).max().item() <= 1e-5
        rm2, rv2 = outs["running_mean0"].clone(), outs["running_var0"].clone()
        ops.bn_stats(out, 1e-5, 0.9, rm2, rv2)      # the stand-alone statistics kernels, which read the activation again
        em = ((outs["running_mean"] - rm2).abs() / sig.float()).max().item()
        ev = ((outs["running_var"] - rv2).abs() / v64.float()).max().item()
        print(f"{name}: running mean {em:.2e}, running var {ev:.2e} (of 1e-5)")
        assert em <= 1e-5 and ev <= 1e-5, "running buffers"


def digests(cases=None):
    """SHA-256 of every output of every case (bitwise comparison of two builds on ONE machine; never committed)"""
    out = {}
    for name, c in (BRANCHES if cases is None else cases).items():
        outs, _ = run_case(name, c)
        for k in ("out", "dw", "mean", "rstd", "planes", "running_mean", "running_var"):
            if k in outs:
                out[f"{name}.{k}"] = hashlib.sha256(outs[k].detach().contiguous().cpu().numpy().tobytes()).hexdigest()
    return out
