"""The one-product fp16 inference plan (FusedVAEInference(precision="f16")) without a GPU: the structure of its launch lists, the host
planner behind its fused epilogue, and a CPU emulation of its arithmetic against the fp64 oracle.

The plans are built with ``_plan_only=True`` over host tensors and never run; the library's support queries are host code."""
import gc
import os
import sys

import pytest
import torch

from tests import f16_emul as E
from tests.util import NORTH_STAR_RTOL, ROOT, rel_err

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_fused_plans as G      # noqa: E402  (its pointer resolver; no case is added to it)

SHAPES = [(3, 128, 128, 32), (1, 32, 16, 4)]      # (C, S, z, B)
CONV_F16 = {"vp_conv5_gather_f16": 11, "vp_conv5_scatter_f16": 10, "vp_conv_gather_f16": 14}      # entry point -> index of `products`
AFFINE_F16 = ("vp_conv5_gather_affine_f16", "vp_conv5_scatter_affine_f16")
# fp16 producer -> the bf16x3 plan's producer at the same place of the list
FMT_OF = {"vp_bn_act_fwd_split_fmt_f32": "vp_bn_act_fwd_split_f32", "vp_nchw_to_nhwc_split_fmt_f32": "vp_nchw_to_nhwc_split_f32",
          "vp_im2col5s2_split_fmt_f32": "vp_im2col5s2_split_f32"}


def _plans(C, S, z, B):
    import vae_play_amd as V
    torch.manual_seed(0)
    vae = V.VAE(S, z, C)
    return vae, {p: V.FusedVAEInference(vae, B, S, C, precision=p, _plan_only=True) for p in ("f16", "bf16x3")}


def _calls(inf):
    """(entry point, arguments without the stream slot, tag) of the encode and decode lists"""
    out = []
    for which in ("encode", "decode"):
        for plan in inf._plans[which]:
            out += [(c[0], c[2][:c[3]], c[5]) for c in plan.calls]
    return out


@pytest.mark.parametrize("C,S,z,B", SHAPES)
def test_plan_structure(C, S, z, B):
    vae, infs = _plans(C, S, z, B)
    f16, bf = infs["f16"], infs["bf16x3"]
    cf, cb = _calls(f16), _calls(bf)
    # the launch-shape rules are shared: the same layers fuse, and the lists pair up launch by launch
    assert f16.fused_layers == bf.fused_layers and f16.unfused_layers == bf.unfused_layers
    assert len(cf) == len(cb)
    L = f16.L
    n16 = 0
    for (nf, af, tf), (nb, ab, tb) in zip(cf, cb):
        assert tf == tb
        if tf.endswith(".fwd") and tf != "fin.fwd":      # every 5x5 layer that use16 admits (all channel counts here are multiples of 8)
            n16 += 1
            assert nf in CONV_F16 or nf in AFFINE_F16, (tf, nf)
            if nf in CONV_F16:
                assert af[CONV_F16[nf]] == 1 and af[CONV_F16[nf] + 1] == 1.0, (tf, af)
                assert tf[:-4] in f16.unfused_layers
            else:
                assert af[-1] == (0 if tf == f"dec{L - 1}.fwd" else 2), (tf, af[-1])      # out_fmt
                assert tf[:-4] in f16.fused_layers
        else:      # the final convolution, the dense layers and the glue: the bf16x3 plan's entry points (producers: their fp16 form)
            assert FMT_OF.get(nf, nf) == nb, (tf, nf, nb)
            if nf in FMT_OF:
                assert af[-1] == 1, (nf, af)                 # VP_SPLIT_F16
    assert n16 == 2 * L
    assert cf[-1][2] == "fin.fwd" or cf[-2][2] == "fin.fwd"
    # the layer feeding the final convolution is fused at these shapes: the out_fmt == 0 branch above was taken
    assert f"dec{L - 1}" in f16.fused_layers
    # weights are packed as fp16 planes (pack format 2) wherever they are split
    jobs = [j for c in f16._prep.calls if c[0] == "vp_pack_w5_batch" for j in c[2][0]]
    assert jobs and all(j.split in (0, 2) for j in jobs) and any(j.split == 2 for j in jobs)

    # every pointer resolves into plan-owned or model memory after a garbage collection
    plans, seen = [("prep", f16._prep)], {}
    for which, ps in f16._plans.items():
        for p in ps:
            seen.setdefault(id(p), (p, which))
    plans += [(w, p) for p, w in seen.values()]
    gc.collect()
    calls, unknown, _ = G.canonical(f16, plans, [("", vae)], {})
    assert unknown == 0 and len(calls) > 10
    assert "infer-f16" not in " ".join(G.CASE_NAMES)


def test_training_plans_refuse_the_mode():
    import vae_play_amd as V
    from vae_play_amd import optim
    from vae_play_amd.engine import FusedVAEStep
    torch.manual_seed(0)
    vae = V.VAE(32, 16, 1)
    opt = optim.Adam(vae.parameters(), lr=1e-4)
    with pytest.raises(ValueError):
        FusedVAEStep(vae, opt, 4, 32, 1, precision="f16", _plan_only=True)
    with pytest.raises(ValueError):
        V.set_conv_precision("f16")


# ---- host planner -------------------------------------------------------------------------------------------------------------
# (family, B, Hs, Cbig, Csmall) of every 5x5 stride-2 block of the inference plans at 128x128x3 batch 32 and 64x64x3 batch 128
INFER_LAYERS = ([(0, 32, 32, 64, 128), (0, 32, 16, 128, 256), (0, 32, 8, 256, 512), (1, 32, 8, 512, 512), (1, 32, 16, 256, 512),
                 (1, 32, 32, 128, 256), (1, 32, 64, 64, 128)]
                + [(0, 128, 16, 64, 128), (0, 128, 8, 128, 256), (1, 128, 8, 256, 256), (1, 128, 16, 128, 256), (1, 128, 32, 64, 128)])
# vp_conv5_affine_supported(family, precision, B, Hs, Hs, Cbig, Csmall, 2) recorded from the parent commit, for the shapes of
# tests/test_gpu_conv_affine.py (its GATHER / SCATTER lists as (family, B, Hs, Cin, Cout), and the refusals of its error-path test)
PARENT = {
    0: {(0, 32, 32, 64, 128): 1, (0, 32, 16, 128, 256): 1, (0, 128, 16, 64, 128): 1, (0, 128, 8, 128, 256): 1,
        (1, 32, 8, 512, 512): 1, (1, 32, 16, 512, 256): 1, (1, 32, 32, 256, 128): 1, (1, 32, 64, 128, 64): 1,
        (1, 128, 8, 256, 256): 1, (1, 128, 16, 256, 128): 1, (1, 128, 32, 128, 64): 1,
        (0, 4, 8, 256, 512): 0, (0, 4, 16, 24, 128): 0},
    1: {(0, 32, 32, 64, 128): 1, (0, 128, 16, 64, 128): 1,
        (1, 32, 8, 512, 512): 1, (1, 32, 16, 512, 256): 1, (1, 32, 32, 256, 128): 1, (1, 32, 64, 128, 64): 1,
        (1, 128, 8, 256, 256): 1, (1, 128, 16, 256, 128): 1, (1, 128, 32, 128, 64): 1,
        (1, 32, 64, 128, 32): 0},
}


def _supported(lib, family, prec, B, Hs, Cin, Cout):
    Cbig, Csmall = (Cin, Cout) if family == 0 else (Cout, Cin)
    return lib.vp_conv5_affine_supported(family, prec, B, Hs, Hs, Cbig, Csmall, 2)


def test_host_planner():
    from vae_play_amd import _lib, ops
    lib = _lib.load()
    for family, B, Hs, Cbig, Csmall in INFER_LAYERS:
        got2, got0 = (lib.vp_conv5_affine_supported(family, p, B, Hs, Hs, Cbig, Csmall, 2) for p in (2, 0))
        assert got2 == got0, (family, B, Hs, Cbig, Csmall, got2, got0)
    assert any(lib.vp_conv5_affine_supported(f, 2, B, Hs, Hs, Cb, Cs, 2) for f, B, Hs, Cb, Cs in INFER_LAYERS)
    for prec, table in PARENT.items():
        for (family, B, Hs, Cin, Cout), want in table.items():
            assert _supported(lib, family, prec, B, Hs, Cin, Cout) == want, (prec, family, B, Hs, Cin, Cout)
    assert lib.vp_conv5_affine_supported(0, 3, 32, 32, 32, 64, 128, 2) == 0 and lib.vp_conv5_affine_supported(0, -1, 32, 32, 32, 64, 128, 2) == 0
    assert ops.conv5_affine_supported(0, "f16", 32, 32, 32, 64, 128, 2) and not ops.conv5_affine_supported(0, "f16", 4, 8, 8, 256, 512, 2)


# ---- CPU emulation of the arithmetic ------------------------------------------------------------------------------------------
def _trained_params(C, S, z, B, L, seed=0):
    """fp64 parameters with non-trivial BatchNorm state, by the recipe of tests/test_gpu_infer.py on the CPU oracle: gamma ~ U(0.5, 1.5),
    beta ~ N(0, 0.2), then three train-mode forwards on seeded batches (momentum moves the running statistics to the data's)"""
    from oracle import ref_cpu as O
    p = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in O.init_params(C, z, L, seed=seed).items()}
    g = torch.Generator().manual_seed(100 + seed)
    for k in p:
        if k.endswith((".bn.weight", "fc.1.weight")):
            p[k] = torch.empty(p[k].shape).uniform_(0.5, 1.5, generator=g).double()
        elif k.endswith((".bn.bias", "fc.1.bias")):
            p[k] = (torch.randn(p[k].shape, generator=g) * 0.2).double()
    with torch.no_grad():
        for j in range(3):
            xb = torch.rand((B, C, S, S), generator=torch.Generator().manual_seed(200 + j)).double()
            eb = torch.randn((B, z), generator=torch.Generator().manual_seed(300 + j)).double()
            O.vae_forward(p, xb, eb, L, training=True)
    return p


@pytest.mark.parametrize("C,S,z,B", [(1, 32, 16, 4), (3, 64, 64, 4)])
def test_emulated_arithmetic_meets_the_contract(C, S, z, B):
    """operands of every 16-bit layer rounded to fp16, everything else fp64, against the unrounded fp64 oracle: <= 1e-3"""
    from oracle import ref_cpu as O
    L = O.iter_level_for(S)
    p = _trained_params(C, S, z, B, L)
    x = torch.rand((B, C, S, S), generator=torch.Generator().manual_seed(7)).double()
    eps = torch.randn((B, z), generator=torch.Generator().manual_seed(8)).double()
    want, got = E.vae_forward(p, x, eps, L, rounded=False), E.vae_forward(p, x, eps, L, rounded=True)
    with torch.no_grad():
        ref = O.vae_forward(p, x, eps, L, training=False)
        dec_want, dec_got = E.decoder_forward(p, want["z"], L, rounded=False), E.decoder_forward(p, want["z"], L, rounded=True)
    assert torch.equal(want["x_tilde"], ref["x_tilde"]) and torch.equal(want["mu"], ref["mu"]), "the emulation without rounding is the oracle"
    errs = {k: rel_err(got[k], want[k]) for k in ("mu", "logvar", "x_tilde")}
    errs["decode"] = rel_err(dec_got, dec_want)
    print(f"f16 emulation {S}x{S}x{C} b{B}: " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert all(v > 0.0 for v in errs.values()), "the rounding did nothing"
    assert all(v <= NORTH_STAR_RTOL for v in errs.values()), errs
