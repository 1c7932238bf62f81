"""Fused segmentation inference (vae_play_amd.infer_be.FusedBEInference, csrc/be_infer.hip) checked without a GPU:

  1. tests/host_emul/be_infer_emul.cpp compiles csrc/be_infer.h -- the text the kernels run -- for the host and runs its tile bodies
     over every tile of each shape of tests/be_infer_ref.SHAPES, against the fp64 oracle at OP_RTOL: the four border rules
     (intermediates and coordinates are 0 outside the image, the resize clamps, partial and tiny tiles);
  2. the packed, BatchNorm-folded parameters applied with torch in fp64 equal the oracle's eval-mode block;
  3. the structure of the launch lists of a plan built over host buffers (``_plan_only=True``, never run; that a second
     ``refresh()`` leaves the lists identical needs a device to run it on: tests/test_gpu_be_infer.py);
  4. header, ctypes table and library agree on the new symbols.
"""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import be_infer_ref as R
from tests.test_infer_gan_plan_cpu import FORBIDDEN, PREP_ONLY
from tests.util import OP_RTOL, ROOT, assert_close

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_emul", "be_infer_emul.cpp")
HDR = os.path.join(ROOT, "vae_play_amd", "csrc", "be_infer.h")
OUT = os.path.join(HERE, "host_emul", "libvp_be_infer_emul.so")
FP, BP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte)
NEW_PREP = ("vp_be_fold_conv_f32", "vp_be_up_pack_f32", "vp_be_predictor_pack_f32")


@pytest.fixture(scope="module")
def emul():
    if (not os.path.exists(OUT)) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        cxx = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    lib.emul_be_up.argtypes = [FP, ctypes.c_size_t, FP, FP] + [ctypes.c_int] * 6
    lib.emul_be_pred.argtypes = [FP, ctypes.c_size_t, FP, FP, BP, ctypes.c_float] + [ctypes.c_int] * 5
    lib.emul_be_up_pack.argtypes = [FP] * 10 + [ctypes.c_float, FP, ctypes.c_int, ctypes.c_int]
    lib.emul_be_pred_pack.argtypes = [FP] * 7 + [ctypes.c_int]
    return lib


def fp(t):
    assert t.is_contiguous() and t.dtype == torch.float32 and t.data_ptr() % 16 == 0
    return ctypes.cast(t.data_ptr(), FP)


def pack_up(emul, p, prefix, cin, cmid):
    out = torch.full((emul.emul_be_up_params_floats(cin, cmid),), float("nan"))
    bn = [p[f"{prefix}conv.{j}.conv.1.{k}"] for j in (0, 1) for k in ("weight", "bias", "running_mean", "running_var")]
    assert emul.emul_be_up_pack(fp(p[prefix + "conv.0.conv.0.weight"]), *map(fp, bn[:4]), fp(p[prefix + "conv.1.conv.0.weight"]),
                                *map(fp, bn[4:]), 1e-5, fp(out), cin, cmid) == 0
    assert not torch.isnan(out).any()
    return out


def pack_pred(emul, p, c):
    out = torch.full((emul.emul_be_pred_params_floats(c),), float("nan"))
    q = [p[f"predictor.{i}.conv.0.{k}"] for i in range(3) for k in ("weight", "bias")]
    assert emul.emul_be_pred_pack(*map(fp, q), fp(out), c) == 0
    assert not torch.isnan(out).any()
    return out


def test_tile_constants_and_support_table(emul):
    from vae_play_amd import infer_be
    assert (emul.emul_be_tile_h(), emul.emul_be_tile_w()) == (R.TH, R.TW) == infer_be.TILE
    ok = {pair for w in infer_be.HEAD_WIDTHS for pair in ((w, w // 4), (w // 4, w // 8))}
    for cin in range(1, 70):
        for cmid in range(1, 20):
            assert bool(emul.emul_be_supported(cin, cmid)) == ((cin, cmid) in ok), (cin, cmid)
    # every tile fits the 64 KiB a workgroup gets without asking for more
    assert max(emul.emul_be_up_lds_floats(ci, cm) for ci, cm in ok) * 4 <= 64 * 1024
    assert max(emul.emul_be_pred_lds_floats(c) for c in (2, 4, 8)) * 4 <= 64 * 1024


# ---- 1. the tile bodies on the host ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", R.SHAPES)
@pytest.mark.parametrize("width", R.WIDTHS)
def test_host_emulation_vs_fp64_oracle(emul, width, h, w):
    """Both Up blocks (the first with ONE input shared by the two heads, head stride 0; the second with an input per head) and the
    predictor with its mask, every tile of the map, against the fp64 oracle of that block."""
    case = R.head_case(width, h, w)
    B, c1, c2 = R.BATCH, width // 4, width // 8
    par1 = torch.stack([pack_up(emul, p, "conv1.", width, c1) for p in case["params"]])
    par2 = torch.stack([pack_up(emul, p, "conv2.", c1, c2) for p in case["params"]])
    par3 = torch.stack([pack_pred(emul, p, c2) for p in case["params"]])
    x = R.nhwc(case["x"])
    y1 = torch.full((2, B, 2 * h, 2 * w, c1), float("nan"))
    assert emul.emul_be_up(fp(x), 0, fp(par1), fp(y1), 2, B, h, w, width, c1) == 0
    x2 = torch.stack([R.nhwc(t) for t in case["u1_in"]])
    y2 = torch.full((2, B, 4 * h, 4 * w, c2), float("nan"))
    assert emul.emul_be_up(fp(x2), x2[0].numel(), fp(par2), fp(y2), 2, B, 2 * h, 2 * w, c1, c2) == 0
    x3 = torch.stack([R.nhwc(t.float()) for t in case["u2"]])
    logits = torch.full((2, B, 1, 4 * h, 4 * w), float("nan"))
    thr = torch.stack(case["logits"]).median().item()
    mask = torch.full((2, B, 1, 4 * h, 4 * w), 7, dtype=torch.uint8)
    assert emul.emul_be_pred(fp(x3), x3[0].numel(), fp(par3), fp(logits), ctypes.cast(mask.data_ptr(), BP), thr, 2, B, 4 * h, 4 * w, c2) == 0
    for k in range(2):
        tag = f"w{width} {h}x{w} head{k}"
        assert_close(y1[k].permute(0, 3, 1, 2), case["u1"][k], OP_RTOL, f"emul up1 {tag}")
        assert_close(y2[k].permute(0, 3, 1, 2), case["u2"][k], OP_RTOL, f"emul up2 {tag}")
        assert_close(logits[k], case["logits"][k], OP_RTOL, f"emul predictor {tag}")
    assert torch.equal(mask.bool(), logits >= thr) and int(mask.max()) <= 1
    # ... and the oracle's mask wherever its logit is not within the kernel's tolerance of the threshold
    ref = torch.stack(case["logits"])
    clear = (ref - thr).abs() > OP_RTOL * ref.abs().max()
    assert torch.equal(mask.bool()[clear], (ref >= thr)[clear])
    if h * w > 1:
        assert 0.2 < mask.float().mean().item() < 0.8, "the threshold should split the logits"
    # without a mask pointer the logits are the same bits
    again = torch.full_like(logits, float("nan"))
    assert emul.emul_be_pred(fp(x3), x3[0].numel(), fp(par3), fp(again), None, thr, 2, B, 4 * h, 4 * w, c2) == 0
    assert torch.equal(again, logits)


def test_the_cases_can_tell_the_border_rules_apart():
    """The oracle itself, with each border rule broken in turn, moves by far more than OP_RTOL on the cases above: they can fail."""
    from oracle import ref_cpu as O
    case = R.head_case(32, R.TH + 1, R.TW + 1)
    p, x = R.f64(case["params"][0]), case["x"].double()
    ref = case["u1"][0]
    scale = ref.abs().max()

    def bn_relu(y, pre):
        return F.relu(F.batch_norm(y, p[pre + "running_mean"], p[pre + "running_var"], p[pre + "weight"], p[pre + "bias"], False, 0.1, 1e-5))

    def up(xc, first_on_padding=False, resize_zero=False):
        w1, w2 = p["conv1.conv.0.conv.0.weight"], p["conv1.conv.1.conv.0.weight"]
        if first_on_padding:            # the first layer evaluated on the padding ring instead of a zero intermediate
            a = bn_relu(F.conv2d(F.pad(xc, (2, 2, 2, 2)), w1), "conv1.conv.0.conv.1.")
            b = bn_relu(F.conv2d(a, w2), "conv1.conv.1.conv.1.")
        else:
            a = bn_relu(F.conv2d(xc, w1, padding=1), "conv1.conv.0.conv.1.")
            b = bn_relu(F.conv2d(a, w2, padding=1), "conv1.conv.1.conv.1.")
        if resize_zero:                 # a zero ring instead of the clamped index
            return F.interpolate(F.pad(b, (1, 1, 1, 1)), scale_factor=2, mode="bilinear")[:, :, 2:-2, 2:-2]
        return F.interpolate(b, scale_factor=2, mode="bilinear")

    xc = O.blocks_add_coords(x)
    assert ((up(xc) - ref).abs().max() / scale).item() <= 1e-12
    # coordinates continued into the padding ring (-1 and W) instead of zeroed
    hh, ww = x.shape[2], x.shape[3]
    big = F.pad(x, (1, 1, 1, 1))
    cont = torch.cat([big, torch.arange(-1, ww + 1.0, dtype=x.dtype).view(1, 1, 1, -1).expand(x.shape[0], 1, hh + 2, ww + 2),
                      torch.arange(-1, hh + 1.0, dtype=x.dtype).view(1, 1, -1, 1).expand(x.shape[0], 1, hh + 2, ww + 2)], 1)
    a = bn_relu(F.conv2d(cont, p["conv1.conv.0.conv.0.weight"]), "conv1.conv.0.conv.1.")
    b = bn_relu(F.conv2d(a, p["conv1.conv.1.conv.0.weight"], padding=1), "conv1.conv.1.conv.1.")
    wrong = {"coordinates continued": F.interpolate(b, scale_factor=2, mode="bilinear"),
             "intermediate on padding": up(xc, first_on_padding=True), "zero ring in the resize": up(xc, resize_zero=True)}
    for what, y in wrong.items():
        e = ((y - ref).abs().max() / scale).item()
        assert e > 100 * OP_RTOL, f"{what}: the case cannot see it ({e:.2e})"


# ---- 2. the fold ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", R.WIDTHS)
def test_packed_parameters_are_the_folded_block(emul, width):
    from oracle import ref_cpu as O
    h, w = 5, 7
    case = R.head_case(width, h, w)
    p, x = case["params"][1], case["x"].double()
    for prefix, cin, cmid, xin, ref in (("conv1.", width, width // 4, x, case["u1"][1]),
                                        ("conv2.", width // 4, width // 8, case["u1_in"][1].double(), case["u2"][1])):
        k1 = cin + 2
        q = pack_up(emul, p, prefix, cin, cmid).double()
        n1, n2 = 9 * k1 * cmid, 9 * cmid * cmid
        t1 = (cmid + 3) // 4 * 4
        w1 = q[:n1].view(3, 3, k1, cmid).permute(3, 2, 0, 1)
        s1 = q[n1:n1 + cmid]
        w2 = q[n1 + t1:n1 + t1 + n2].view(3, 3, cmid, cmid).permute(3, 2, 0, 1)
        o2 = n1 + t1 + (n2 + 3) // 4 * 4
        s2 = q[o2:o2 + cmid]
        assert q.numel() == o2 + t1
        y = F.relu(F.conv2d(O.blocks_add_coords(xin), w1, s1, padding=1))
        y = F.interpolate(F.relu(F.conv2d(y, w2, s2, padding=1)), scale_factor=2, mode="bilinear")
        assert_close(y, ref, OP_RTOL, f"fold {prefix} width {width}")
    # the predictor's block holds the reference's numbers themselves, re-ordered
    c = width // 8
    q = pack_pred(emul, p, c)
    o = 0
    for i, (ci, co) in enumerate(((c, 2 * c), (2 * c, c), (c, 1))):
        wt, bs = p[f"predictor.{i}.conv.0.weight"], p[f"predictor.{i}.conv.0.bias"]
        assert torch.equal(q[o:o + 9 * ci * co].view(3, 3, ci, co).permute(3, 2, 0, 1), wt)
        o += (9 * ci * co + 3) // 4 * 4
        assert torch.equal(q[o:o + co], bs)
        o += (co + 3) // 4 * 4
    assert o == q.numel()


# ---- 3. the plan ------------------------------------------------------------------------------------------------------------------
def _calls(inf, which):
    return [c for plan in inf._plans[which] for c in plan.calls]


def _names(inf, which):
    return [c[0] for c in _calls(inf, which)]


@pytest.mark.parametrize("kind", ("be", "gan"))
def test_plan_structure(kind):
    import vae_play_amd as V
    from vae_play_amd import _lib
    net = R.seeded_net(kind)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    B, h, w = 2, 9, 17
    inf = V.FusedBEInference(net, B, h, w, _plan_only=True)
    aux = net.aux_convs if kind == "gan" else net.feature_net.aux_convs
    width = 64 if kind == "gan" else 32
    assert inf.precision == "f32" and inf.width == width and len(aux) == (4 if kind == "gan" else 6)
    convs = ["vp_conv_gather_f32"] * len(aux)
    tail = ["vp_be_up_infer_f32", "vp_be_up_infer_f32", "vp_be_predictor_infer_f32"]
    assert _names(inf, "predict.cl") == convs + tail and len(_names(inf, "predict.cl")) == len(aux) + 3
    assert _names(inf, "predict") == ["vp_nchw_to_nhwc_f32"] + convs + tail
    assert _names(inf, "features.cl") == convs and _names(inf, "features") == ["vp_nchw_to_nhwc_f32"] + convs
    assert set(inf._plans) == {"features", "predict", "segment", "features.cl", "predict.cl", "segment.cl"}
    for which in inf._plans:
        for c in _calls(inf, which):
            name, args, side = c[0], c[2], c[6]
            assert name in _lib.SIGNATURES and len(args) == len(_lib.SIGNATURES[name][1]), name
            assert side is None, f"{name}: inference plans are single-stream"
            assert not any(f in name for f in FORBIDDEN), f"{which}: {name} is a training launch"
            assert not any(name.startswith(f) for f in PREP_ONLY + NEW_PREP), f"{which}: {name} belongs to refresh()"
    prep = [c[0] for c in inf._prep.calls]
    assert set(prep) == {"vp_be_fold_conv_f32", "vp_pack_w_f32", "vp_be_up_pack_f32", "vp_be_predictor_pack_f32"}
    assert prep.count("vp_be_fold_conv_f32") == prep.count("vp_pack_w_f32") == len(aux)
    assert prep.count("vp_be_up_pack_f32") == 4 and prep.count("vp_be_predictor_pack_f32") == 2
    for c in inf._prep.calls:
        assert len(c[2]) == len(_lib.SIGNATURES[c[0]][1]) and c[6] is None, c[0]
    # the chain of buffers: layer i reads what layer i - 1 wrote; the first reads the input where it lies (channels_last) or its copy
    cl, nc = _calls(inf, "predict.cl"), _calls(inf, "predict")
    assert cl[0][2][0].value == inf.x_in.data_ptr() and nc[1][2][0].value == inf.x_nhwc.data_ptr()
    assert nc[0][2][0].value == inf.x_in.data_ptr() and nc[0][2][1].value == inf.x_nhwc.data_ptr()
    assert all(a[2][1:-1] == b[2][1:-1] for a, b in zip(cl[:1], nc[1:2])) and all(a is b or a[2] is b[2] for a, b in zip(cl[1:], nc[2:]))
    for i in range(1, len(aux)):
        assert cl[i][2][0].value == cl[i - 1][2][3].value
        assert cl[i][2][4:14] == [B, h, w, h, w, aux[i].conv[0].weight.shape[1], aux[i].conv[0].weight.shape[0], aux[i].conv[0].kernel_size, 1, 1]
    up1, up2, pred = (c[2] for c in cl[len(aux):])
    c1, c2 = width // 4, width // 8
    assert up1[0].value == cl[len(aux) - 1][2][3].value == inf.feat.data_ptr() and up1[1] == 0, "both heads read the one feature map"
    assert up1[4:10] == [2, B, h, w, width, c1]
    assert up2[0].value == up1[3].value and up2[1] == B * 2 * h * 2 * w * c1 and up2[4:10] == [2, B, 2 * h, 2 * w, c1, c2]
    assert pred[0].value == up2[3].value and pred[1] == B * 4 * h * 4 * w * c2 and pred[6:11] == [2, B, 4 * h, 4 * w, c2]
    assert pred[3].value == inf.logits.data_ptr() and pred[4] is None
    # segment = predict but for the predictor's mask pointer and threshold
    for sfx in ("", ".cl"):
        a, b = _calls(inf, "predict" + sfx), _calls(inf, "segment" + sfx)
        assert all(x is y for x, y in zip(a[:-1], b[:-1]))
        pa, pb = a[-1][2], b[-1][2]
        assert a[-1][0] == b[-1][0] and [i for i in range(len(pa) - 1) if getattr(pa[i], "value", pa[i]) != getattr(pb[i], "value", pb[i])] == [4, 5]
        assert pb[4].value == inf.masks.data_ptr() and pb[5] == 0.5 and inf.masks.dtype == torch.uint8
    # building the plan wrote nothing to the module and left its mode alone
    assert not net.training and all(torch.equal(v, before[k]) for k, v in net.state_dict().items())


def test_bf16x3_plan_adds_only_the_operand_splits():
    """"bf16x3" changes the aux_convs layers alone: the existing split-operand convolution reads split planes and writes fp32, so each
    layer's input is split first -- the one launch per layer an "f32" plan does not have; the weights are split in refresh()."""
    import vae_play_amd as V
    net = R.seeded_net("be")
    inf = V.FusedBEInference(net, 2, 3, 5, precision="bf16x3", _plan_only=True)
    n = len(net.feature_net.aux_convs)
    assert _names(inf, "predict.cl") == ["vp_split_f32", "vp_conv_gather_bf16x3"] * n + ["vp_be_up_infer_f32"] * 2 + ["vp_be_predictor_infer_f32"]
    prep = [c[0] for c in inf._prep.calls]
    assert prep.count("vp_pack_w_split") == n and "vp_pack_w_f32" not in prep
    f32 = V.FusedBEInference(net, 2, 3, 5, _plan_only=True)
    assert _names(inf, "predict.cl")[2 * n:] == _names(f32, "predict.cl")[n:]
    with pytest.raises(ValueError, match="precision"):
        V.FusedBEInference(net, 2, 3, 5, precision="f16", _plan_only=True)


def test_unsupported_width_and_normalised_coordinates_are_refused():
    import vae_play_amd as V
    from vae_play_amd import networks_BE
    torch.manual_seed(0)
    net = networks_BE.ComposeNet(networks_BE.FeatureNet(None, 96, 24))
    with pytest.raises(ValueError, match=r"24.*\(16, 32, 64\)"):
        V.FusedBEInference(net, 2, 4, 4, _plan_only=True)
    net = R.seeded_net("be")
    net.mask_net.conv2.add_coord.if_normalize = True
    with pytest.raises(ValueError, match="if_normalize"):
        V.FusedBEInference(net, 2, 4, 4, _plan_only=True)
    with pytest.raises(ValueError, match="positive"):
        V.FusedBEInference(R.seeded_net("be"), 0, 4, 4, _plan_only=True)


# ---- 4. the ABI -------------------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from tests.test_abi import header_functions
    from vae_play_amd import _lib
    lib = _lib.load()
    counts = {"vp_be_infer_supported": 2, "vp_be_up_params_floats": 2, "vp_be_predictor_params_floats": 1, "vp_be_up_pack_f32": 15,
              "vp_be_predictor_pack_f32": 9, "vp_be_fold_conv_f32": 11, "vp_be_up_infer_f32": 11, "vp_be_predictor_infer_f32": 12}
    for n, k in counts.items():
        assert n in header_functions() and n in _lib.SIGNATURES and hasattr(lib, n), n
        assert len(_lib.SIGNATURES[n][1]) == k, n
    assert lib.vp_be_infer_supported(64, 16) == 1 and lib.vp_be_infer_supported(24, 6) == 0
    assert lib.vp_be_up_params_floats(24, 6) == 0 and lib.vp_be_predictor_params_floats(3) == 0
