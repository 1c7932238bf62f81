"""Fused Style-GAN inference (vae_play_amd.infer_stylegan.FusedStyleGanInference, csrc/stylegan_infer.hip) checked without a GPU:
header, ctypes table and library agree on the new symbols; the two-pass form of the twin-SCSE kernel and the folded MLP are the
reference's arithmetic in fp64; the structure of the launch lists of plans built over host buffers (``_plan_only=True``, never run);
what the constructor refuses."""
import collections
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import stylegan_infer_ref as R
from tests.util import ROOT

NEW = ("vp_scse2_workspace_bytes", "vp_scse2_preferred", "vp_scse2_fwd_f32", "vp_cat2_nhwc_f32", "vp_sg_out_params_floats",
       "vp_sg_out_tanh_preferred", "vp_sg_out_pack_f32", "vp_sg_out_tanh_f32")
# entries that move data without computing.  The three slices that stay de-interleave the [B][2 z] rows of the one dense launch behind
# fc_mu / fc_logvar into the dense mu, logvar (and z = mu) that vp_latent_fwd_f32 and the MLP read: B x z floats each.
COPIES = ("vp_slice_channels_f32", "vp_nhwc_to_nchw_f32", "vp_add_coords_f32", "vp_split_pad_f32")
SLICES = {"enc.mu", "enc.logvar", "z.mu"}
MY_CONVS = ("conv1", "conv2", "down1", "down2", "down3", "down4")


def _lib():
    from vae_play_amd import _lib
    return _lib, _lib.load()


def test_header_table_and_library_agree_on_the_new_symbols():
    _l, lib = _lib()
    header = open(os.path.join(ROOT, "include", "vaeplay_hip.h")).read()
    for name in NEW:
        assert name in _l.SIGNATURES, name
        assert re.search(r"\b%s\(" % name, header), f"{name} is not declared in include/vaeplay_hip.h"
        assert getattr(lib, name) is not None
    import vae_play_amd as V
    assert V.FusedStyleGanInference.__name__ in V.__all__
    assert lib.vp_sg_out_params_floats(32) == 27 * 32 + 4 and lib.vp_sg_out_params_floats(6) == 0 and lib.vp_sg_out_params_floats(260) == 0
    # the workspace: two partial planes of nchunk rows and two gates; 0 for sizes the kernel refuses
    assert lib.vp_scse2_workspace_bytes(2, 35, 32, 8) == (2 * 2 * 1 * 32 + 2 * 2 * 32) * 4
    assert lib.vp_scse2_workspace_bytes(0, 35, 32, 8) == 0 and lib.vp_scse2_workspace_bytes(2, 35, 32, 33) == 0


@pytest.mark.parametrize("case", range(len(R.SCSE2_CASES)))
def test_two_pass_identity_in_fp64(case):
    """mean_p y_a = c_a mean_p x + mean_p (x s_a): the two-pass form equals scse(scse(x)) on signed data"""
    x, sd, ref = R.scse2_case(case)
    with torch.no_grad():
        for relu in (0, 1):
            got = R.scse2_two_pass(R.f64(sd), x.double(), relu)
            assert (got - ref[relu]).abs().max().item() <= 1e-12 * max(1.0, ref[relu].abs().max().item())
    assert bool((x < 0).any()) and bool((ref[1] == 0).any()) and bool((ref[0] < 0).any())


@pytest.mark.parametrize("S", R.SIZES)
def test_folded_mlp_is_the_three_layers_in_fp64(S):
    """W3 W2 W1 and W3 (W2 b1 + b2) + b3, in the order the plan's prep list forms them"""
    G, _, _ = R.seeded_nets(S)
    (w1, b1), (w2, b2), (w3, b3) = ((blk.fc[0].weight.detach().double(), blk.fc[0].bias.detach().double()) for blk in G.mlp.model)
    z = torch.randn((5, R.Z), generator=R.gen(9), dtype=torch.float64)
    want = F.linear(F.linear(F.linear(z, w1, b1), w2, b2), w3, b3)
    w21, b21 = w2 @ w1, w2 @ b1 + b2
    got = F.linear(z, w3 @ w21, w3 @ b21 + b3)
    assert got.shape == (5, S * S) and (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def _plan(S, prec):
    import vae_play_amd as V
    G, E, D = R.seeded_nets(S)
    return V.FusedStyleGanInference(G, E, D, batch_size=R.BATCH, precision=prec, _plan_only=True), (G, E, D)


@pytest.mark.parametrize("prec", ("f32", "bf16x3"))
@pytest.mark.parametrize("S", R.SIZES)
def test_plan_structure(S, prec):
    _l, lib = _lib()
    B = R.BATCH
    nets = R.seeded_nets(S)
    flags = [{n: m.training for n, m in net.named_modules()} for net in nets]
    inf, (G, E, D) = _plan(S, prec)
    assert inf.S == S and [{n: m.training for n, m in net.named_modules()} for net in nets] == flags
    modes = ("blend", "c0", "c1")
    want = {f"generate.{m}{cl}" for m in modes for cl in ("", ".cl")}
    want |= {f"stylize.{m}{e}{cl}" for m in modes for e in ("", ".eps") for cl in ("", ".cl")}
    want |= {"encode", "encode.cl", "discriminate", "discriminate.cl"}
    assert set(inf._plans) == want
    for which, lists in inf._plans.items():
        calls = [c for plan in lists for c in plan.calls]
        names = [c[0] for c in calls]
        by_layer = collections.defaultdict(list)
        for name, fn, args, slot, flops, tag, side, sargs in calls:
            assert fn is not None and tag, f"{which}: {name} has no tag"
            assert name in _l.SIGNATURES and len(args) == len(_l.SIGNATURES[name][1]) and side is None, name
            if any(name.startswith(c) for c in COPIES):
                assert name == "vp_slice_channels_f32" and tag in SLICES, f"{which}: {name} ({tag}) is a copy"
            assert name == "vp_cat2_nhwc_f32" or "_cat" not in name, f"{which}: {name} is a concatenation"
            assert not name.startswith("vp_pack_") and "pack" not in name and "fold" not in name and tag != "gen.mlp.fold", \
                f"{which}: {name} ({tag}) belongs to refresh()"
            if name == "vp_nchw_to_nhwc_f32":
                assert tag == "xs.nhwc", tag
            by_layer[tag.rsplit(".", 1)[0]].append(name)
        kind = which.split(".")[0]
        if kind in ("generate", "stylize"):
            mode = which.split(".")[1]
            t = f"gen.{mode}"
            # the style plane is ONE dense launch over the folded map (or the three layers where the predicate says so)
            n_dense = sum(1 for c in calls if c[5].startswith("gen.mlp"))
            assert n_dense == (1 if inf.folded else 3)
            assert names.count("vp_cat2_nhwc_f32") == 1
            for layer in MY_CONVS:
                m = getattr(G, layer)
                C, cin = m.conv_1.conv[0].weight.shape[:2]
                got = by_layer[f"{t}.{layer}"]
                gathers = [c for c in calls if c[5] == f"{t}.{layer}.fwd"]
                assert len(gathers) == 1 and gathers[0][0] == ("vp_conv_gather_f32" if prec == "f32" or cin % 8 else "vp_conv_gather_bf16x3")
                cout = gathers[0][2][10]            # Csmall of the gather entry
                if mode == "blend":
                    assert cout == 2 * C and got.count("vp_pair_blend_fwd_f32") == 1 and not any(n.startswith("vp_instnorm") for n in got)
                else:
                    assert cout == C and "vp_pair_blend_fwd_f32" not in got
                    assert sum(n.startswith("vp_instnorm_act_fwd") for n in got) == (1 if m.bn == "instance" else 0)
                assert [n for n in got if n not in ("vp_split_f32", "vp_pair_blend_fwd_f32") and not n.startswith(("vp_conv_gather", "vp_instnorm"))] == []
            if mode != "blend":
                assert "vp_pair_blend_fwd_f32" not in names
            size = S // 16
            for k in (1, 2, 3):
                up = getattr(G, f"up{k}")
                C = up.up_convs[0].weight.shape[1]
                size *= 2
                # the two InstanceNorms write the two channel slices of cat_convs.0's input: row stride 2C, second slice C floats in
                cat_in = inf._bufs[f"{t}.up{k}.cat.x"]
                (up_in,) = [c for c in calls if c[5] == f"{t}.up{k}.up_convs.in"]
                assert up_in[0] == "vp_instnorm_act_fwd_ld_f32" and up_in[2][1].value == cat_in.data_ptr() and up_in[2][2] == 2 * C
                skip = [c for c in calls if c[5] in (f"{t}.skip{k}.in", f"{t}.skip{k}.fwd") and c[0] in ("vp_instnorm_act_fwd_ld_f32", "vp_conv_in_act_f32")]
                assert len(skip) == 1
                dst = skip[0][2][1] if skip[0][0] == "vp_instnorm_act_fwd_ld_f32" else skip[0][2][2]
                ldy = skip[0][2][2] if skip[0][0] == "vp_instnorm_act_fwd_ld_f32" else skip[0][2][3]
                assert dst.value == cat_in.data_ptr() + 4 * C and ldy == 2 * C
                # cat_convs.0 is one gather with bias and ReLU in the epilogue
                got = by_layer[f"{t}.up{k}.cat_convs.0"]
                assert [n for n in got if n != "vp_split_f32"] == ["vp_conv_gather_f32" if prec == "f32" else "vp_conv_gather_bf16x3"]
                (g0,) = [c for c in calls if c[5] == f"{t}.up{k}.cat_convs.0.fwd"]
                assert g0[2][2] is not None and g0[2][13] == 1 and g0[2][9] == 2 * C and g0[2][10] == C
                # and the block ends in one vp_scse2_fwd_f32, or in two vp_scse_fwd_f32 where the predicate says so
                tail = by_layer[f"{t}.up{k}.cat_convs"] + by_layer[f"{t}.up{k}.cat_convs.scse"]
                if lib.vp_scse2_preferred(B, size * size, C, C // 4):
                    assert tail == ["vp_scse2_fwd_f32"]
                else:
                    assert tail == ["vp_scse_fwd_f32"] * 2
            assert names[-1] == "vp_sg_out_tanh_f32" or names[-3:] == ["vp_conv_gather_f32", "vp_act_fwd_f32", "vp_nhwc_to_nchw_f32"]
        if kind == "stylize":
            # the encoder list, one launch that writes z where the MLP reads it, the generator list
            cl = ".cl" if which.endswith(".cl") else ""
            enc, gen = inf._plans["encode" + cl], inf._plans[f"generate.{which.split('.')[1]}" + cl]
            assert lists[:len(enc)] == enc and lists[len(enc) + 1:] == gen and len(lists) == len(enc) + 1 + len(gen)
            (zc,) = lists[len(enc)].calls
            assert zc[0] == ("vp_latent_fwd_f32" if ".eps" in which else "vp_slice_channels_f32")
            assert zc[2][3 if ".eps" in which else 1].value == inf.z.data_ptr()
        if kind == "encode":
            assert names.count("vp_gemm_f32") == 1 and names.count("vp_nchw_to_nhwc_f32") == (0 if which.endswith(".cl") else 1)
        if kind == "discriminate":
            assert names[0] == "vp_cat2_nhwc_f32" and names[-1] == "vp_twin_head_fwd_f32" and names.count("vp_twin_head_fwd_f32") == 1
    for c in inf._prep.calls:
        assert c[0] in _l.SIGNATURES and len(c[2]) == len(_l.SIGNATURES[c[0]][1]) and c[6] is None, c[0]
    # the stacked weights are built by refresh(): one pair per myConv2d of the blended lists, the two fc heads
    assert len(inf._stacks) == 6 + 2 + 2           # six weights, conv1 / conv2 biases, fc weight and bias
    if inf.folded:
        assert [c[0] for c in inf._prep.calls if c[5] == "gen.mlp.fold"] == ["vp_gemm_f32"] * 4


def test_methods_need_their_net():
    import vae_play_amd as V
    from vae_play_amd import _lib as L
    G, _, _ = R.seeded_nets(32)
    inf = V.FusedStyleGanInference(G, batch_size=2, _plan_only=True)
    assert set(inf._plans) == {f"generate.{m}{cl}" for m in ("blend", "c0", "c1") for cl in ("", ".cl")}
    x = torch.zeros((2, 3, 32, 32))
    for call in (lambda: inf.encode_style(x), lambda: inf.stylize(x, x, 0), lambda: inf.discriminate(x, x)):
        with pytest.raises(L.VaePlayHipError, match="built without one"):
            call()


def test_constructor_refusals():
    import vae_play_amd as V
    from vae_play_amd import network_Style_GAN as N
    G, E, D = R.seeded_nets(32)
    with pytest.raises(ValueError, match="Generator"):
        V.FusedStyleGanInference(torch.nn.Linear(2, 2), batch_size=3, _plan_only=True)
    with pytest.raises(ValueError, match="StyleEncoder"):
        V.FusedStyleGanInference(G, D, None, batch_size=3, _plan_only=True)
    with pytest.raises(ValueError, match="Discriminator"):
        V.FusedStyleGanInference(G, E, E, batch_size=3, _plan_only=True)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="batch_size"):
            V.FusedStyleGanInference(G, E, D, batch_size=bad, _plan_only=True)
    with pytest.raises(ValueError, match="precision"):
        V.FusedStyleGanInference(G, E, D, batch_size=3, precision="f16", _plan_only=True)
    for S in (16, 48):
        with pytest.raises(ValueError, match="power of two"):
            V.FusedStyleGanInference(N.Generator(S, 8, ), batch_size=3, _plan_only=True)
    E64, D64 = R.seeded_nets(64)[1:]
    with pytest.raises(ValueError, match="image_size"):
        V.FusedStyleGanInference(G, E64, None, batch_size=3, _plan_only=True)
    with pytest.raises(ValueError, match="image_size"):
        V.FusedStyleGanInference(G, None, D64, batch_size=3, _plan_only=True)
    with pytest.raises(ValueError, match="z_dim"):
        V.FusedStyleGanInference(G, N.StyleEncoder(4, 32), None, batch_size=3, _plan_only=True)
