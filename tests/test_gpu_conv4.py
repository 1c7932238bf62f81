"""4x4 convolutions on the device (kernel 4, padding 1, stride 1 | 2: myConv2d(.., 4, 2) and nn.ConvTranspose2d(in, out, 4, 2, 1) of
models/network_Style_GAN.py:49,95-98,116):

  a. the C ABI vp_conv_{gather,scatter,wgrad}_{f32,bf16x3} (and the fp16-pair forms) at ks = 4 against the fp64 direct sums of
     tests/conv_ref.py, |out - r| <= tau(K, mode) * A with conv_ref's tau -- no tolerance of its own; outputs pre-filled with NaN, so
     that a pixel the scatter family's phase grid misses shows;
  b. the bias epilogue vp_conv_scatter_bias_*: direct sum + bias, bit-equal to vp_conv_scatter_* without one, and exactly the bias
     where no tap reaches;
  c. the autograd front end functional.conv2d (ks 4) and functional.conv_transpose2d against the same direct sums;
  d. the reference-generated fixtures (tools/gen_golden_conv4.py): blocks.Conv2d(8, 16, 4, 2, bn="instance"), the bare transposed
     convolution and StyleUp(16, 8).
Every test prints its figures before it asserts."""
import pytest
import torch

from tests import conv_ref as R
from tests.util import NORTH_STAR_RTOL, assert_close, load_golden, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = 4
NAN = float("nan")


def _nhwc(B, C, H, W, gen):
    return torch.randn(B, H, W, C, device=DEV, generator=gen).permute(0, 3, 1, 2)


def _nan_cl(B, C, H, W):
    return torch.full((B, H, W, C), NAN, device=DEV).permute(0, 3, 1, 2)


def _check(report, label, mode, got, r, A, K):
    assert not torch.isnan(got).any(), f"{label} {mode}: sampled outputs that the kernel never wrote"
    ratio, i, err = R.worst_scaled(got, r, A, R.tau(K, mode).to(r.device))
    report.append(f"{label}[{mode}] {ratio:.3f}")
    print(f"  {label}[{mode}] worst err/tau {ratio:.3f} (|out - r| = {err:.2e} * A, K = {int(K.flatten()[i])})")
    assert ratio <= 1.0, f"{label} {mode}: |out - r| = {err:.2e} * A at flat sample {i} exceeds tau(K = {int(K.flatten()[i])})"


def _check_families(report, mode, big, small, w, stride, gather, scatter, dw, seed, gather_bias=None, scatter_bias=None):
    """gather (big -> small), scatter (small -> big) and the weight gradient of one layer against the direct sums; None skips one"""
    B, Cb, Hb, Wb = big.shape
    _, Cs, Hs, Ws = small.shape
    if gather is not None:
        gp = R.gather_points(B, Hs, seed, Ws=Ws)
        r, A, K = R.gather_ref(big, w, gp, stride, terms=True)
        if gather_bias is not None:
            r, A, K = r + gather_bias.double(), A + gather_bias.double().abs(), K + 1
        _check(report, "gather", mode, R.take(gather, gp), r, A, K)
    if scatter is not None:
        assert not torch.isnan(scatter).any(), f"scatter {mode}: pixels of the big side never written"
        sp = R.scatter_points(B, Hb, seed, Wb=Wb)
        r, A, K = R.scatter_ref(small, w, sp, stride, terms=True)
        if scatter_bias is not None:
            r, A, K = r + scatter_bias.double(), A + scatter_bias.double().abs(), K + 1
        _check(report, "scatter", mode, R.take(scatter, sp), r, A, K)
    if dw is not None:
        cs, cb = R.tile_channels(Cs), R.tile_channels(Cb)
        _check(report, "wgrad", mode, dw[cs][:, cb], *R.wgrad_ref(big, small, cs, cb, KS, stride, terms=True))


# ---- a. the C ABI ---------------------------------------------------------------------------------------------------------
# (B, Cb, Cs, Hb, Wb, stride): a 128-tile edge and an M tail | phase grid larger than the small grid | stride 1 | scalar path (f32 only)
# | the three tap-pair kinds of the weight gradient | down4 / up1 channels at batch 2
SHAPES = [(3, 64, 136, 12, 20, 2), (2, 16, 8, 13, 9, 2), (2, 8, 24, 9, 7, 1), (2, 3, 5, 10, 6, 2), (2, 32, 64, 16, 16, 2),
          (2, 64, 128, 16, 16, 2), (2, 64, 64, 16, 16, 2), (2, 256, 256, 32, 32, 2)]
ABI = ([(s, "f32") for s in SHAPES] + [(s, "bf16x3") for s in SHAPES if s[1] % 8 == 0 and s[2] % 8 == 0]
       + [(s, "f16x2/3") for s in SHAPES[:2]])
GSCALE = 16.0


def _operands(shape, seed):
    B, Cb, Cs, Hb, Wb, stride = shape
    gen = torch.Generator(device=DEV).manual_seed(seed)
    Hs, Ws = R.out_size(Hb, KS, stride), R.out_size(Wb, KS, stride)
    big, small = _nhwc(B, Cb, Hb, Wb, gen), _nhwc(B, Cs, Hs, Ws, gen)
    w = torch.randn(Cs, Cb, KS, KS, device=DEV, generator=gen) * 0.05
    return big, small, w, Hs, Ws


def _run_abi(shape, mode, big, small, w, Hs, Ws):
    """gather, scatter (onto NaN) and weight gradient through the C ABI in `mode`"""
    from vae_play_amd import _lib, ops
    B, Cb, Cs, Hb, Wb, stride = shape
    S = ops._stream()
    geom = (B, Hs, Ws, Hb, Wb)
    gather, scatter = _nan_cl(B, Cs, Hs, Ws), _nan_cl(B, Cb, Hb, Wb)
    dw = torch.full((Cs, Cb, KS, KS), NAN, device=DEV)
    if mode == "f32":
        p0, p1 = ops.pack_w(w, True, True)
        _lib.call("vp_conv_gather_f32", ops._p(big), ops._p(p0), None, ops._p(gather), *geom, Cb, Cs, KS, stride, 0, S)
        _lib.call("vp_conv_scatter_f32", ops._p(small), ops._p(p1), ops._p(scatter), *geom, Cs, Cb, KS, stride, S)
        ws = ops._ws(_lib.load().vp_conv_wgrad_workspace_bytes(*geom, Cb, Cs, KS, stride), big)
        _lib.call("vp_conv_wgrad_f32", ops._p(big), ops._p(small), ops._p(dw), *geom, Cb, Cs, KS, stride, ops._p(ws), ws.numel() * 4, S)
    elif mode == "bf16x3":
        p0, p1 = ops.pack_w_split(w, True, True)
        bs, ss = ops.split_f32(big), ops.split_f32(small)
        _lib.call("vp_conv_gather_bf16x3", ops._pv(bs), ops._pv(p0), None, ops._p(gather), *geom, Cb, Cs, KS, stride, 0, S)
        _lib.call("vp_conv_scatter_bf16x3", ops._pv(ss), ops._pv(p1), ops._p(scatter), *geom, Cs, Cb, KS, stride, S)
        ws = ops._ws(_lib.load().vp_conv_wgrad_bf16x3_workspace_bytes(*geom, Cb, Cs, KS, stride), big)
        _lib.call("vp_conv_wgrad_bf16x3", ops._pv(bs), ops._pv(ss), ops._p(dw), *geom, Cb, Cs, KS, stride, ops._p(ws), ws.numel() * 4, S)
    else:       # fp16-pair planes, three products; the packed weights are split in the same format
        p0, p1 = ops.pack_w(w, True, True)
        bs, ss, p0s, p1s = (ops.split_f32(v, ops.SPLIT_F16) for v in (big, small, p0, p1))      # (named: alive until the launches ran)
        _lib.call("vp_conv_gather_f16", ops._pv(bs), ops._pv(p0s), None, ops._p(gather), *geom, Cb, Cs, KS, stride, 0, 3, 1.0, S)
        _lib.call("vp_conv_scatter_f16", ops._pv(ss), ops._pv(p1s), ops._p(scatter), *geom, Cs, Cb, KS, stride, 3, 1.0, S)
        dw = None
    torch.cuda.synchronize()
    return gather, scatter, dw


@pytest.mark.parametrize("shape,mode", ABI, ids=[f"{'x'.join(map(str, s))}-{m.replace('/', '_')}" for s, m in ABI])
def test_c_abi_k4_matches_the_direct_sum(shape, mode):
    seed = sum(shape) + len(mode)
    big, small, w, Hs, Ws = _operands(shape, seed)
    gather, scatter, dw = _run_abi(shape, mode, big, small, w, Hs, Ws)
    report = []
    print(f"direct-sum err/tau C ABI ks=4 {shape} {mode}:")
    _check_families(report, mode, big, small, w, shape[5], gather, scatter, dw, seed)


@pytest.mark.parametrize("shape", SHAPES[:2], ids=["x".join(map(str, s)) for s in SHAPES[:2]])
def test_c_abi_k4_wgrad_f16x2(shape):
    """vp_conv_wgrad_f16x2 (two products: the big operand keeps its fp16 hi plane) against the direct sum, and against the
    operation with that operand rounded to fp16 -- its declared arithmetic"""
    from vae_play_amd import _lib, ops
    B, Cb, Cs, Hb, Wb, stride = shape
    seed = sum(shape)
    big, small, w, Hs, Ws = _operands(shape, seed)
    geom = (B, Hs, Ws, Hb, Wb, Cb, Cs, KS, stride)
    dw = torch.full((Cs, Cb, KS, KS), NAN, device=DEV)
    ws = ops._ws(_lib.load().vp_conv_wgrad_bf16x3_workspace_bytes(*geom), big)
    bs, ss = ops.split_f32(big, ops.SPLIT_F16), ops.split_f32(small, ops.SPLIT_F16, GSCALE)
    _lib.call("vp_conv_wgrad_f16x2", ops._pv(bs), ops._pv(ss), ops._p(dw), *geom, 1.0 / GSCALE, ops._p(ws), ws.numel() * 4, ops._stream())
    torch.cuda.synchronize()
    cs, cb = R.tile_channels(Cs), R.tile_channels(Cb)
    report = []
    print(f"direct-sum err/tau vp_conv_wgrad_f16x2 ks=4 {shape}:")
    _check(report, "wgrad", "f16x2/2", dw[cs][:, cb], *R.wgrad_ref(big, small, cs, cb, KS, stride, terms=True))
    _check(report, "wgrad", "f16x2/2 declared", dw[cs][:, cb], *R.wgrad_ref(big.half().float(), small, cs, cb, KS, stride, terms=True))


@pytest.mark.parametrize("shape,mode", [(SHAPES[4], "bf16x3"), (SHAPES[5], "bf16x3"), (SHAPES[0], "bf16x3"), (SHAPES[0], "f32")],
                         ids=["pairs64x64", "pairs128x128", "tails", "f32"])
def test_wgrad_k4_is_bit_identical_over_two_runs(shape, mode):
    big, small, w, Hs, Ws = _operands(shape, 5)
    a = _run_abi(shape, mode, big, small, w, Hs, Ws)[2]
    b = _run_abi(shape, mode, big, small, w, Hs, Ws)[2]
    assert not torch.isnan(a).any() and torch.equal(a, b)


# ---- b. the bias epilogue of the scatter family -------------------------------------------------------------------------------
def _scatter_bias(mode, small, w, bias, Hb, Wb, stride, ks=KS):
    from vae_play_amd import ops
    out_shape = (small.shape[0], w.shape[1], Hb, Wb)
    if mode == "f32":
        _, p1 = ops.pack_w(w, False, True)
        return ops.conv_scatter_bias(small, p1, bias, ks, stride, Hb, Wb), ops.conv_scatter(small, p1, ks, stride, Hb, Wb), out_shape
    _, p1 = ops.pack_w_split(w, False, True)
    ss = ops.split_f32(small)
    return (ops.conv_scatter_bias_bf16x3(ss, tuple(small.shape), p1, bias, w.shape[1], ks, stride, Hb, Wb),
            ops.conv_scatter_bf16x3(ss, tuple(small.shape), p1, w.shape[1], ks, stride, Hb, Wb), out_shape)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[2]], ids=["tile_edge", "odd", "stride1"])
def test_scatter_bias_is_direct_sum_plus_bias(shape, mode):
    B, Cb, Cs, Hb, Wb, stride = shape
    seed = sum(shape) + 1
    big, small, w, Hs, Ws = _operands(shape, seed)
    bias = torch.randn(Cb, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    with_bias, plain, out_shape = _scatter_bias(mode, small, w, bias, Hb, Wb, stride)
    none_bias = _scatter_bias(mode, small, w, None, Hb, Wb, stride)[0]
    torch.cuda.synchronize()
    assert tuple(with_bias.shape) == out_shape
    assert torch.equal(none_bias, plain), "a null bias must give the bits of vp_conv_scatter_*"
    report = []
    print(f"direct-sum err/tau scatter_bias ks=4 {shape} {mode}:")
    _check_families(report, mode, big, small, w, stride, None, with_bias, None, seed, scatter_bias=bias)
    _check_families(report, mode, big, small, w, stride, None, plain, None, seed)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_scatter_bias_where_no_tap_reaches(mode):
    """ks = 1, stride 2: only the even pixels of the big side receive a product; all the others hold exactly the bias"""
    B, Cb, Cs, Hb, Wb = 2, 16, 8, 7, 10
    gen = torch.Generator(device=DEV).manual_seed(3)
    Hs, Ws = R.out_size(Hb, 1, 2), R.out_size(Wb, 1, 2)
    small = _nhwc(B, Cs, Hs, Ws, gen)
    w = torch.randn(Cs, Cb, 1, 1, device=DEV, generator=gen)
    bias = torch.randn(Cb, device=DEV, generator=gen)
    out = _scatter_bias(mode, small, w, bias, Hb, Wb, 2, ks=1)[0]
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    reached = torch.zeros(Hb, Wb, dtype=torch.bool, device=DEV)
    reached[::2, ::2] = True
    expect = bias.view(1, Cb, 1, 1).expand(B, Cb, Hb, Wb)
    assert torch.equal(out[:, :, ~reached], expect[:, :, ~reached]), "pixels no tap reaches must hold exactly the bias"
    sp = R.scatter_points(B, Hb, 3, Wb=Wb)
    r, A, K = R.scatter_ref(small, w, sp, 2, terms=True)
    _check([], "scatter", mode, R.take(out, sp), r + bias.double(), A + bias.double().abs(), K + 1)


# ---- c. the autograd front end ------------------------------------------------------------------------------------------------
def _with_precision(mode):
    from vae_play_amd import functional as FH

    class _Ctx:
        def __enter__(self):
            self.prev = FH.get_conv_precision()
            FH.set_conv_precision(mode)

        def __exit__(self, *a):
            FH.set_conv_precision(self.prev)
    return _Ctx()


def _dbias(report, db, dy):
    B, C, H, W = dy.shape
    _check(report, "dbias", "f32", db[None], dy.double().sum((0, 2, 3))[None], dy.double().abs().sum((0, 2, 3))[None],
           torch.full((1, C), B * H * W, device=DEV))


# (B, Cin, Cout, H, W, stride): odd sizes at both strides, and a channel count the bf16x3 path zero-pads to a multiple of 8
CONV2D = [(2, 16, 24, 13, 9, 2), (2, 8, 16, 9, 7, 1), (2, 6, 16, 10, 14, 2)]


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("B,Cin,Cout,H,W,stride", CONV2D, ids=["odd_s2", "odd_s1", "padded_s2"])
def test_functional_conv2d_k4(B, Cin, Cout, H, W, stride, mode):
    from vae_play_amd import functional as FH
    seed = B + Cin + Cout + H + W + stride
    gen = torch.Generator(device=DEV).manual_seed(seed)
    with _with_precision(mode):
        x = _nhwc(B, Cin, H, W, gen).requires_grad_(True)
        w = (torch.randn(Cout, Cin, KS, KS, device=DEV, generator=gen) * (2.0 / (Cin * 16)) ** 0.5).requires_grad_(True)
        b = (torch.randn(Cout, device=DEV, generator=gen) * 0.1).requires_grad_(True)
        y = FH.conv2d(x, w, b, stride)
        Hs, Ws = R.out_size(H, KS, stride), R.out_size(W, KS, stride)
        assert tuple(y.shape) == (B, Cout, Hs, Ws)
        dy = _nhwc(B, Cout, Hs, Ws, gen)
        y.backward(dy)
        torch.cuda.synchronize()
    report = []
    print(f"direct-sum err/tau functional.conv2d ks=4 {(B, Cin, Cout, H, W, stride)} {mode}:")
    _check_families(report, mode, x.detach(), dy, w.detach(), stride, y.detach(), x.grad, w.grad, seed, gather_bias=b.detach())
    _dbias(report, b.grad, dy)


# (B, Cin, Cout, Hs, Ws, feed): "norm" = the input is an InstanceNorm + ReLU output (carries split planes in bf16x3 mode)
CONVT = [(2, 16, 8, 5, 7, "plain"), (3, 64, 32, 8, 12, "plain"), (2, 5, 3, 4, 6, "plain")]
CONVT_CASES = [(*c, m) for c in CONVT for m in ("f32", "bf16x3")] + [(2, 16, 8, 5, 7, "norm", "bf16x3")]


@pytest.mark.parametrize("B,Cin,Cout,Hs,Ws,feed,mode", CONVT_CASES, ids=[f"{c[1]}to{c[2]}-{c[5]}-{c[6]}" for c in CONVT_CASES])
def test_functional_conv_transpose2d(B, Cin, Cout, Hs, Ws, feed, mode):
    from vae_play_amd import functional as FH
    seed = B + Cin + Cout + Hs + Ws
    gen = torch.Generator(device=DEV).manual_seed(seed)
    use16 = mode == "bf16x3" and Cin % 8 == 0 and Cout % 8 == 0
    with _with_precision(mode):
        x0 = _nhwc(B, Cin, Hs, Ws, gen).requires_grad_(True)
        x = FH.instance_norm_act(x0, 1e-5, "relu") if feed == "norm" else x0
        if feed == "norm":
            assert getattr(x, "_vp_split", None) is not None, "the normalisation's output must carry split planes"
            x.retain_grad()
        w = (torch.randn(Cin, Cout, KS, KS, device=DEV, generator=gen) * (2.0 / (Cin * 4)) ** 0.5).requires_grad_(True)
        b = torch.randn(Cout, device=DEV, generator=gen).requires_grad_(True)
        y = FH.conv_transpose2d(x, w, b, 2)
        assert tuple(y.shape) == (B, Cout, 2 * Hs, 2 * Ws)
        dy = _nhwc(B, Cout, 2 * Hs, 2 * Ws, gen)
        y.backward(dy)
        y_nobias = FH.conv_transpose2d(x.detach(), w.detach(), None, 2)
        torch.cuda.synchronize()
    report = []
    tm = "bf16x3" if use16 else "f32"
    print(f"direct-sum err/tau functional.conv_transpose2d {(B, Cin, Cout, Hs, Ws, feed)} {mode}:")
    # big = y / dy, small = x / dx: forward is the scatter (+ bias), dx the gather of dy, dW the weight gradient with big = dy
    _check_families(report, tm, dy, x.detach(), w.detach(), 2, x.grad, y.detach(), w.grad, seed, scatter_bias=b.detach())
    _check_families(report, tm, dy, x.detach(), w.detach(), 2, None, y_nobias, None, seed)
    _dbias(report, b.grad, dy)


def test_conv_transpose2d_honours_needs_input_grad():
    from vae_play_amd import functional as FH
    gen = torch.Generator(device=DEV).manual_seed(9)
    x = _nhwc(2, 16, 4, 6, gen)
    w = torch.randn(16, 8, KS, KS, device=DEV, generator=gen).requires_grad_(True)
    b = torch.randn(8, device=DEV, generator=gen)
    FH.conv_transpose2d(x, w, b, 2).sum().backward()
    assert x.grad is None and b.grad is None and w.grad is not None
    with pytest.raises(ValueError):
        FH.conv_transpose2d(x, torch.randn(16, 8, 5, 5, device=DEV), None, 2)
    with pytest.raises(ValueError):
        FH.conv_transpose2d(x, w, None, 1)


# ---- d. reference-generated fixtures ------------------------------------------------------------------------------------------
def _tols(mode):
    return (1e-4, 3e-4) if mode == "f32" else (NORTH_STAR_RTOL, NORTH_STAR_RTOL)


def _load_params(mod, g):
    sd = {k[len("param/"):]: t(v) for k, v in g.items() if k.startswith("param/")}
    res = mod.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return mod.to(DEV).train()


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_fixture_conv2d_k4s2_instance_relu(mode):
    from vae_play_amd import blocks
    g = load_golden("stylegan_conv2d_k4s2_instance_relu")
    ty, tg = _tols(mode)
    with _with_precision(mode):
        mod = _load_params(blocks.Conv2d(8, 16, 4, 2, bn="instance"), g)
        for tag in ("even", "odd"):
            mod.zero_grad(set_to_none=True)
            x = t(g[f"{tag}/x"]).to(DEV).requires_grad_(True)
            y = mod(x)
            y.backward(t(g[f"{tag}/gy"]).to(DEV))
            torch.cuda.synchronize()
            errs = {"y": assert_close(y, t(g[f"{tag}/y"]), ty, f"{tag} y"), "dx": assert_close(x.grad, t(g[f"{tag}/dx"]), tg, f"{tag} dx")}
            for k, p in mod.named_parameters():
                errs[k] = assert_close(p.grad, t(g[f"{tag}/grad/{k}"]), tg, f"{tag} grad {k}")
            print(f"fixture conv2d k4s2 {tag} {mode}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_fixture_conv_transpose_k4s2(mode):
    from vae_play_amd.network_Style_GAN import ConvTranspose2d
    g = load_golden("stylegan_convt_k4s2")
    ty, tg = _tols(mode)
    with _with_precision(mode):
        mod = _load_params(ConvTranspose2d(16, 8, 4, 2, 1), g)
        x = t(g["x"]).to(DEV).requires_grad_(True)
        y = mod(x)
        y.backward(t(g["gy"]).to(DEV))
        torch.cuda.synchronize()
    errs = {"y": assert_close(y, t(g["y"]), ty, "y"), "dx": assert_close(x.grad, t(g["dx"]), tg, "dx")}
    for k, p in mod.named_parameters():
        errs[k] = assert_close(p.grad, t(g["grad/" + k]), tg, "grad " + k)
    print(f"fixture convT k4s2 {mode}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_fixture_styleup_16to8(mode):
    """up_convs.0.bias.grad is rounding noise in the reference too (InstanceNorm removes a per-channel shift: 1.8e-6 beside weight
    gradients of order 10), so it is only held to max|db| <= 1e-4 * max|dW|; the bare-convT fixture holds a real bias gradient."""
    from vae_play_amd.network_Style_GAN import StyleUp
    g = load_golden("stylegan_up_16to8")
    ty, tg = _tols(mode)
    with _with_precision(mode):
        mod = _load_params(StyleUp(16, 8), g)
        x, skip = (t(g[k]).to(DEV).requires_grad_(True) for k in ("x", "skip"))
        y = mod(x, skip)
        y.backward(t(g["gy"]).to(DEV))
        torch.cuda.synchronize()
    grads = dict(mod.named_parameters())
    db, dW = grads["up_convs.0.bias"].grad, grads["up_convs.0.weight"].grad
    print(f"fixture StyleUp {mode}: max|db| {db.abs().max().item():.2e}, max|dW| {dW.abs().max().item():.2e} "
          f"(reference {abs(g['grad/up_convs.0.bias']).max():.2e}, {abs(g['grad/up_convs.0.weight']).max():.2e})")
    errs = {"y": assert_close(y, t(g["y"]), ty, "y"), "dx": assert_close(x.grad, t(g["dx"]), tg, "dx"),
            "dskip": assert_close(skip.grad, t(g["dskip"]), tg, "dskip")}
    for k, p in grads.items():
        if k != "up_convs.0.bias":
            errs[k] = assert_close(p.grad, t(g["grad/" + k]), tg, "grad " + k)
    print(f"fixture StyleUp {mode}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert db.abs().max().item() <= 1e-4 * dW.abs().max().item()
