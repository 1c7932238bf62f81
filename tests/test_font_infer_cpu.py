"""Fused font U-Net inference (vae_play_amd.infer_font.FusedFontInference, csrc/font_infer.hip) checked without a GPU: header, ctypes
table and library agree on the new symbols; ``vp_conv_in_supported`` answers as DESIGN.md 11.1 states; the structure of the launch
lists of plans built over host buffers (``_plan_only=True``, never run); what the constructor refuses."""
import collections
import os
import re

import pytest

from tests import font_infer_ref as R
from tests.util import ROOT

NEW = ("vp_conv_in_supported", "vp_conv_in_preferred", "vp_conv_in_pack_f32", "vp_conv_in_act_f32", "vp_font_pred_params_floats", "vp_font_pred_pack_f32",
       "vp_font_pred_infer_f32", "vp_font_relay_input_f32", "vp_font_attn1_f32", "vp_upsample2x_bilinear_fwd_ld_f32",
       "vp_instnorm_act_fwd_ld_f32")
# entries that move data without computing: a concatenation or a layout copy has to be one of these (the two transposes that stay are
# the caller's NCHW image and the relay output, whose (C,H,W) order the dense layer fixes)
COPIES = ("vp_slice_channels_f32", "vp_nhwc_to_nchw_f32", "vp_add_coords_f32", "vp_split_pad_f32")
TRANSPOSES = {"x.nhwc", "relay.nhwc"}


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
    assert V.FusedFontInference.__name__ in V.__all__


def test_conv_in_supported_answers_as_specified():
    _, lib = _lib()
    ok = lib.vp_conv_in_supported
    # every combination the kernel has to take: output maps of 16 / 64 / 256 pixels, the three (ks, stride) pairs, Cin % 64, Cout
    for side in (4, 8, 16):
        for ks, stride in ((3, 1), (3, 2), (1, 1)):
            for cin in range(64, 1025, 64):
                for cout in (64, 128, 256, 512):
                    assert ok(side * stride, side * stride, cin, cout, ks, stride) == 1, (side, ks, stride, cin, cout)
    assert ok(2, 8, 64, 64, 3, 1) == 1                      # 16 pixels that are not a square
    # refused: Ho*Wo = 512, 48, 1024; ks = 5; stride 2 on a 1x1; a stride-3 layer; channel counts off the grid; nonsense sizes
    for bad in ((16, 32, 64, 64, 3, 1), (6, 8, 64, 64, 3, 1), (32, 32, 64, 64, 3, 1), (8, 8, 64, 64, 5, 1), (8, 8, 64, 64, 1, 2),
                (12, 12, 64, 64, 3, 3), (8, 8, 3, 64, 3, 1), (8, 8, 32, 64, 3, 1), (8, 8, 96, 64, 3, 1), (8, 8, 1088, 64, 3, 1),
                (8, 8, 64, 32, 3, 1), (8, 8, 64, 1, 3, 1), (8, 8, 64, 80, 3, 1), (0, 8, 64, 64, 3, 1), (8, -8, 64, 64, 3, 1),
                (8, 8, 0, 64, 3, 1), (8, 8, 64, 0, 3, 1), (64, 64, 64, 64, 3, 2)):
        assert ok(*bad) == 0, bad
    # the plan's subset: supported and K = ks*ks*Cin <= 576 (the layers the kernel was measured faster on)
    pref = lib.vp_conv_in_preferred
    for args, want in (((4, 4, 64, 64, 3, 1), 1), ((32, 32, 64, 128, 3, 2), 1), ((4, 4, 256, 256, 1, 1), 1), ((16, 16, 576, 64, 1, 1), 1),
                       ((16, 16, 640, 64, 1, 1), 0), ((8, 8, 128, 128, 3, 1), 0), ((8, 8, 1024, 512, 3, 1), 0), ((8, 8, 64, 64, 5, 1), 0),
                       ((16, 32, 64, 64, 3, 1), 0), ((8, 8, 3, 64, 3, 1), 0)):
        assert pref(*args) == want and (ok(*args) == 1 or not want), args
    assert lib.vp_font_pred_params_floats(64) == 9 * 64 + 4 and lib.vp_font_pred_params_floats(6) == 0


@pytest.mark.parametrize("prec", ("f32", "bf16x3"))
@pytest.mark.parametrize("S", (16, 32, 64))
def test_plan_structure(S, prec):
    import vae_play_amd as V
    _l, lib = _lib()
    net = R.seeded_net(S)
    flags = {n: m.training for n, m in net.named_modules()}
    inf = V.FusedFontInference(net, 3, prec, _plan_only=True)
    assert inf.S == S and {n: m.training for n, m in net.named_modules()} == flags
    assert set(inf._plans) == {w + s for w in ("predict", "segment") for s in ("", ".cl", ".y", ".y.cl")} | {"condition", "condition.cl",
                                                                                                           "condition.y"}
    ins, bns = R.in_layers(net, S)
    for which, lists in inf._plans.items():
        calls = [c for plan in lists for c in plan.calls]
        by_layer = collections.defaultdict(list)
        for name, fn, args, slot, flops, tag, side, sargs in calls:
            assert fn is not None and tag, f"{which}: {name} has no tag"
            assert name in _l.SIGNATURES and len(args) == len(_l.SIGNATURES[name][1]) and side is None, name
            assert not any(name.startswith(c) for c in COPIES) and "cat" not in name, f"{which}: {name} is a concatenation or a copy"
            assert not name.startswith("vp_pack_") and "fold" not in name, f"{which}: {name} belongs to refresh()"
            if name == "vp_nchw_to_nhwc_f32":
                assert tag in TRANSPOSES, tag
            by_layer[tag.rsplit(".", 1)[0]].append(name)
        if which.startswith("condition"):
            continue
        # the heads end in ONE entry
        assert calls[-1][0] == "vp_font_pred_infer_f32" and [c[0] for c in calls].count("vp_font_pred_infer_f32") == 1
        assert (calls[-1][2][4] is None) == which.startswith("predict")
        for tag, cin, cout, ks, stride, H in ins:
            if ".y" in which and tag.startswith("style_encoder"):
                assert tag not in by_layer
                continue
            got = by_layer[tag]
            if lib.vp_conv_in_preferred(H, H, cin, cout, ks, stride):
                assert got == ["vp_conv_in_act_f32"], (which, tag, got)
            elif prec == "f32":
                assert len(got) == 2 and got[0] == "vp_conv_gather_f32" and got[1].startswith("vp_instnorm_act_fwd"), (which, tag, got)
            else:       # split operands: at most one vp_split_f32 in front of the pair; a 3-channel input stays exact fp32
                want = "vp_conv_gather_f32" if cin % 8 else "vp_conv_gather_bf16x3"
                assert got[-2] == want and got[-1].startswith("vp_instnorm_act_fwd") and got[:-2] in ([], ["vp_split_f32"]), (which, tag, got)
        for tag in bns:
            got = by_layer[tag]
            if prec == "f32":
                assert got == ["vp_conv_gather_f32"], (which, tag, got)
            else:
                assert got[-1] == "vp_conv_gather_bf16x3" and got[:-1] in ([], ["vp_split_f32"]), (which, tag, got)
        # the resize of every Up and every skip block write into the cat block's input: no pass of their own joins them
        for k in range(len(net.up)):
            assert by_layer[f"up.{k}"] == ["vp_upsample2x_bilinear_fwd_ld_f32"]
    # at least one layer of every net here takes the whole-image kernel, and at S = 64 the two largest levels do not
    taken = [t for t, cin, cout, ks, st, H in ins if lib.vp_conv_in_preferred(H, H, cin, cout, ks, st)]
    assert taken and (S < 64 or {"down.0", "down.1.1", "skip.0", "cat.1"}.isdisjoint(taken))
    for c in inf._prep.calls:
        assert c[0] in _l.SIGNATURES and len(c[2]) == len(_l.SIGNATURES[c[0]][1]) and c[6] is None, c[0]


def test_constructor_refusals():
    import torch
    import vae_play_amd as V
    from vae_play_amd import networks_BE
    net = R.seeded_net(16)
    with pytest.raises(ValueError, match="ComposeNet"):
        V.FusedFontInference(torch.nn.Linear(2, 2), 3, _plan_only=True)
    with pytest.raises(ValueError, match="ComposeNet"):
        V.FusedFontInference(networks_BE.ComposeNet(networks_BE.FeatureNet(None, 256, 32)), 3, _plan_only=True)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="batch_size"):
            V.FusedFontInference(net, bad, _plan_only=True)
    with pytest.raises(ValueError, match="precision"):
        V.FusedFontInference(net, 3, "f16", _plan_only=True)
