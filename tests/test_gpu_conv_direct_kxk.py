"""k x k convolutions (ks 1 | 3 | 5, stride 1 | 2, padding (ks - 1) // 2) against fp64 direct sums of their definition
(tests/conv_ref.py) at their launch shapes: sampled outputs at both borders, in every stride phase, at the channel-tile edges and on
every tap, held to |out - r| <= tau(K) * A with tau from the arithmetic (conv_ref.tau).  Three routes:

  a. the autograd front end (functional.conv2d and conv5x5: the small3 VALU kernels, zero-padded channel counts, split planes handed
     over by a BatchNorm or InstanceNorm in both directions, the 5x5 edge kernels, the split-bf16 and exact-f32 tile kernels) per
     layer of the BE heads, BE-GAN, font and VAE-GAN models at their bench shape, with a coverage test that every convolution those
     models launch is in the table;
  b. the C ABI vp_conv_{gather,scatter,wgrad}_{f32,bf16x3} at shapes that run each internal path once;
  c. the fused steps' first layer: im2col + a 1x1 layer, and the weight gradient through vp_unpack_dw_im2col5_f32.
Operands are generated on the device; every test prints its worst err / tau per family."""
import pytest
import torch

from tests import conv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _nhwc(B, C, H, W, gen):
    """a logical NCHW tensor in NHWC storage, generated on the device"""
    return torch.randn(B, H, W, C, device=DEV, generator=gen).permute(0, 3, 1, 2)


def _check(report, label, mode, got, r, A, K):
    """|got - r| <= tau(K, mode) * A on every sample; records the worst err / tau under `label`"""
    ratio, i, err = R.worst_scaled(got, r, A, R.tau(K, mode).to(r.device))
    report.append(f"{label}[{mode}] {ratio:.3f}")
    assert ratio <= 1.0, f"{label} {mode}: |out - r| = {err:.2e} * A at flat sample {i} exceeds tau(K = {int(K.flatten()[i])})"


def _families(report, mode, x, y, w, stride, gather, scatter, dw, seed, bias=None):
    """gather (+ bias), scatter and weight gradient of one layer against the direct sums; x big side, y small side"""
    B, Cb, Hb, Wb = x.shape
    _, Cs, Hs, Ws = y.shape
    gp, sp = R.gather_points(B, Hs, seed, Ws=Ws), R.scatter_points(B, Hb, seed, Wb=Wb)
    r, A, K = R.gather_ref(x, w, gp, stride, terms=True)
    if bias is not None:
        r, A, K = r + bias.double(), A + bias.double().abs(), K + 1
    _check(report, "gather", mode, R.take(gather, gp), r, A, K)
    _check(report, "scatter", mode, R.take(scatter, sp), *R.scatter_ref(y, w, sp, stride, terms=True))
    cs, cb = R.tile_channels(Cs), R.tile_channels(Cb)
    _check(report, "wgrad", mode, dw[cs][:, cb], *R.wgrad_ref(x, y, cs, cb, w.shape[-1], stride, terms=True))


# ---- a. the autograd front end at the bench launch shapes ------------------------------------------------------------------------------
# (row, layer, Cin, Cout, ks, stride, H_in, B, bias): every distinct convolution of
#   be_heads  ComposeNet(FeatureNet(None, in_channels=256, target_out_channels=32)) on a (16, 256, 64, 64) feature map
#             (tools/bench_be_heads.py: 256 px targets, batch 16); MaskNet and EdgeNet have the same shapes
#   be_gan    ComposeNet(3, 256, feature_channels=256) on (16, 256, 64, 64) and Discriminator(3, 256, 5) on 256 px
#             (tools/bench_be_gan.py); both MaskMappers have the same shapes
#   font      networks_BE_font.ComposeNet(256) with and without the embedding input (generator and style-encoder phases of
#             tools/bench_font.py) and Discriminator(256, 2, 143), 8 images (BASELINE config 5's per-GPU shard); the self-attention
#             q / k / v convolutions run on 1 x 1 maps; layers of equal shape (k and q, the label and style encoders, the mask
#             and edge heads, the discriminator's middle stages and the style encoder's) are listed once
#   vaegan    VaeGan(128) at 16 images: the encoder's 5x5 convolutions, the decoder's last one and the discriminator's, which sees
#             the 48 images of (x, x_tilde, x_p) in one pass (functional.conv5x5; the other rows run functional.conv2d)
# Dispatch at these shapes: functional._Conv (family "conv2d") sends 3x3 stride-1 layers with Cin <= 36, Cout <= 8 to the exact-fp32 small3 kernels in
# both modes (ids *_small3); in bf16x3 mode the other layers run on the split-bf16 kernels, zero-padded to a multiple of 8 on the side
# whose channel count is not one (66 and 2 and 3 in, 1 out; ids *_padded), and in f32 mode on the exact-fp32 tile kernels.
# functional._Conv (family "conv5x5") in bf16x3 mode: the first encoder conv on its im2col as a 1x1 layer (and, its image requiring a gradient, the
# padded scatter), the decoder's 64 -> 1 on the edge kernels (vp_conv5_smallout_bf16x3 forward, vp_conv5_smallin_dgrad_bf16x3,
# vp_conv5_smallout_wgrad_bf16x3), the discriminator's 1 -> 32 on vp_conv5_smallin_fwd_bf16x3 with its input gradient on the
# flipped-tap vp_conv5_smallout_bf16x3; in f32 mode the narrow kernels.  The model runs these two edge layers with a sigmoid / ReLU
# epilogue; here they run without one, on the same kernels, so that the output is the bare sum.
FRONT = [("be_heads", "aux0_1x1", 256, 128, 1, 1, 64, 16, True), ("be_heads", "aux1_3x3", 128, 128, 3, 1, 64, 16, True),
         ("be_heads", "aux2_1x1", 128, 64, 1, 1, 64, 16, True), ("be_heads", "aux3_3x3", 64, 64, 3, 1, 64, 16, True),
         ("be_heads", "aux4_1x1", 64, 32, 1, 1, 64, 16, True), ("be_heads", "aux5_3x3", 32, 32, 3, 1, 64, 16, True),
         ("be_heads", "up1a_coords_small3", 34, 8, 3, 1, 64, 16, True), ("be_heads", "up1b_small3", 8, 8, 3, 1, 64, 16, True),
         ("be_heads", "up2a_coords_small3", 10, 4, 3, 1, 128, 16, True), ("be_heads", "up2b_small3", 4, 4, 3, 1, 128, 16, True),
         ("be_heads", "pred0_small3", 4, 8, 3, 1, 256, 16, True), ("be_heads", "pred1_small3", 8, 4, 3, 1, 256, 16, True),
         ("be_heads", "pred2_small3", 4, 1, 3, 1, 256, 16, True),
         ("be_gan", "aux0_1x1", 256, 128, 1, 1, 64, 16, True), ("be_gan", "aux1_3x3", 128, 128, 3, 1, 64, 16, True),
         ("be_gan", "aux2_1x1", 128, 64, 1, 1, 64, 16, True), ("be_gan", "aux3_3x3", 64, 64, 3, 1, 64, 16, True),
         ("be_gan", "up1a_coords_padded", 66, 16, 3, 1, 64, 16, True), ("be_gan", "up1b_3x3", 16, 16, 3, 1, 64, 16, True),
         ("be_gan", "up2a_coords_small3", 18, 8, 3, 1, 128, 16, True), ("be_gan", "up2b_small3", 8, 8, 3, 1, 128, 16, True),
         ("be_gan", "pred0_3x3", 8, 16, 3, 1, 256, 16, True), ("be_gan", "pred1_small3", 16, 8, 3, 1, 256, 16, True),
         ("be_gan", "pred2_small3", 8, 1, 3, 1, 256, 16, True),
         ("be_gan", "disc_conv0_s2_padded", 2, 16, 3, 2, 256, 16, True), ("be_gan", "disc_conv1_s2", 16, 32, 3, 2, 128, 16, True),
         ("be_gan", "disc_feat0_s2", 32, 64, 3, 2, 64, 16, True), ("be_gan", "disc_feat0b", 64, 64, 3, 1, 32, 16, True),
         ("be_gan", "disc_feat1_s2", 64, 64, 3, 2, 32, 16, True), ("be_gan", "disc_feat1b", 64, 64, 3, 1, 16, 16, True),
         ("be_gan", "disc_pool_1x1", 64, 64, 1, 1, 16, 16, True),
         ("font", "attn_qk_1x1_on_1px", 256, 32, 1, 1, 1, 8, True), ("font", "attn_v_1x1_on_1px", 256, 256, 1, 1, 1, 8, True),
         ("font", "down0_padded", 3, 64, 3, 1, 256, 8, False), ("font", "down1_s2", 64, 128, 3, 2, 256, 8, False),
         ("font", "down1b", 128, 128, 3, 1, 128, 8, False), ("font", "down2_s2", 128, 256, 3, 2, 128, 8, False),
         ("font", "down2b", 256, 256, 3, 1, 64, 8, False), ("font", "down3_s2", 256, 512, 3, 2, 64, 8, False),
         ("font", "down3b", 512, 512, 3, 1, 32, 8, False), ("font", "down4_s2", 512, 512, 3, 2, 32, 8, False),
         ("font", "down4b", 512, 512, 3, 1, 16, 8, False), ("font", "down5_s2", 512, 512, 3, 2, 16, 8, False),
         ("font", "down5b", 512, 512, 3, 1, 8, 8, False), ("font", "down6_s2", 512, 512, 3, 2, 8, 8, False),
         ("font", "down6b", 512, 512, 3, 1, 4, 8, False),
         ("font", "cat5", 1024, 512, 3, 1, 8, 8, False), ("font", "cat4", 1024, 512, 3, 1, 16, 8, False),
         ("font", "cat3", 1024, 512, 3, 1, 32, 8, False), ("font", "up2a", 512, 256, 3, 1, 32, 8, False),
         ("font", "up2b", 256, 256, 3, 1, 32, 8, False), ("font", "cat2", 512, 256, 3, 1, 64, 8, False),
         ("font", "up1a", 256, 128, 3, 1, 64, 8, False), ("font", "up1b", 128, 128, 3, 1, 64, 8, False),
         ("font", "cat1", 256, 128, 3, 1, 128, 8, False), ("font", "up0a", 128, 64, 3, 1, 128, 8, False),
         ("font", "up0b", 64, 64, 3, 1, 128, 8, False), ("font", "skip0_and_heads", 64, 64, 3, 1, 256, 8, False),
         ("font", "cat0", 128, 64, 3, 1, 256, 8, False), ("font", "head_out_padded", 64, 1, 3, 1, 256, 8, True),
         ("font", "style0_s2_padded", 3, 64, 3, 2, 256, 8, False), ("font", "style1_s2_and_disc1", 64, 128, 3, 2, 128, 8, False),
         ("font", "style2_s2_and_disc2", 128, 256, 3, 2, 64, 8, False), ("font", "style3_s2", 256, 256, 3, 2, 32, 8, False),
         ("font", "style4_s2", 256, 256, 3, 2, 16, 8, False), ("font", "style5_s2", 256, 256, 3, 2, 8, 8, False),
         ("font", "style6_1x1", 256, 256, 1, 1, 4, 8, False), ("font", "disc0_s2_padded", 2, 64, 3, 2, 256, 8, False),
         ("font", "disc3_s2", 256, 512, 3, 2, 32, 8, False), ("font", "disc4_s2", 512, 1024, 3, 2, 16, 8, False),
         ("vaegan", "enc0_im2col", 1, 64, 5, 2, 128, 16, False), ("vaegan", "enc1", 64, 128, 5, 2, 64, 16, False),
         ("vaegan", "enc2", 128, 256, 5, 2, 32, 16, False), ("vaegan", "enc3", 256, 512, 5, 2, 16, 16, False),
         ("vaegan", "dec_out_edge_smallout", 64, 1, 5, 1, 128, 16, True),
         ("vaegan", "disc0_edge_smallin", 1, 32, 5, 1, 128, 48, True), ("vaegan", "disc1", 32, 64, 5, 2, 128, 48, False),
         ("vaegan", "disc2", 64, 128, 5, 2, 64, 48, False), ("vaegan", "disc3", 128, 256, 5, 2, 32, 48, False),
         ("vaegan", "disc4", 256, 512, 5, 2, 16, 48, False)]


def _entry(row):
    return "conv5x5" if row == "vaegan" else "conv2d"


def _small3(Cin, Cout, ks, stride, H, B):
    """does functional._Conv run this layer on the exact-fp32 small3 kernels (in both modes)?"""
    from vae_play_amd import ops
    return ks == 3 and stride == 1 and ops.conv3_small_wgrad_applicable(B, H, H, Cin, Cout)


def _norm_act(row, t):
    """the normalisation that hands a layer its input in the row's models: InstanceNorm + ReLU in the font U-Net, else BatchNorm + ReLU;
    in bf16x3 mode its output (and, backwards, its input gradient) carries split planes when the channel count is a multiple of 8"""
    from vae_play_amd import functional as FH
    C = t.shape[1]
    if row == "font":
        return FH.instance_norm_act(t, 1e-5, "relu")
    return FH.batch_norm_act(t, torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV),
                             torch.ones(C, device=DEV), True, 0.1, 1e-5, "relu")


# "plain": fresh operands in both modes.  "split_planes" (bf16x3, layers that do not run small3): the input is a normalisation's output
# that carries split planes, and the output gradient dy is a normalisation's input gradient that carries them, the way the blocks hand
# both over (functional._split_of) -- on each side whose channel count is a multiple of 8.
def _reads_split_planes(row, layer, Cin, Cout, ks, stride, H, B, bias):
    """does the layer's bf16x3 dispatch read split planes of its input or output gradient?  Not the small3 layers (fp32 VALU
    kernels; checked in the test) nor the VAE-GAN edge layers (their kernels read fp32)"""
    if row == "vaegan":
        return stride == 2 or (Cin % 8 == 0 and Cout % 8 == 0)
    return (Cin % 8 == 0 or Cout % 8 == 0) and not layer.endswith("_small3")


FRONT_CASES = ([(*l, m, "plain") for l in FRONT for m in ("f32", "bf16x3")]
               + [(*l, "bf16x3", "split_planes") for l in FRONT if _reads_split_planes(*l)])


@pytest.mark.parametrize("row,layer,Cin,Cout,ks,stride,H,B,bias,mode,feed", FRONT_CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[9]}-{c[10]}" for c in FRONT_CASES])
def test_front_end_layer_matches_the_direct_sum(row, layer, Cin, Cout, ks, stride, H, B, bias, mode, feed):
    """functional.conv2d / conv5x5 forward and backward at the layer's launch shape: y, dx, dW and db against the direct sums"""
    from vae_play_amd import functional as FH
    seed = sum(map(ord, row + layer + mode + feed))
    gen = torch.Generator(device=DEV).manual_seed(seed)
    small3 = _entry(row) == "conv2d" and _small3(Cin, Cout, ks, stride, H, B)
    assert not (small3 and feed != "plain"), "small3 reads the fp32 tensors only"
    tau_mode = "small3" if small3 else mode          # the small3 kernels are exact fp32 in both modes
    prev = FH.get_conv_precision()
    FH.set_conv_precision(mode)
    try:
        x0 = _nhwc(B, Cin, H, H, gen).requires_grad_(True)
        w = (torch.randn(Cout, Cin, ks, ks, device=DEV, generator=gen) * (2.0 / (Cin * ks * ks)) ** 0.5).requires_grad_(True)
        b = (torch.randn(Cout, device=DEV, generator=gen) * 0.1).requires_grad_(True) if bias else None
        split_in = feed == "split_planes" and Cin % 8 == 0
        x = _norm_act(row, x0) if split_in else x0
        if split_in:
            assert getattr(x, "_vp_split", None) is not None, "the normalisation's output must carry split planes"
        x.retain_grad()
        y = FH.conv5x5(x, w, b, stride, None) if _entry(row) == "conv5x5" else FH.conv2d(x, w, b, stride)
        Hs = R.out_size(H, ks, stride)
        assert tuple(y.shape) == (B, Cout, Hs, Hs)
        if feed == "split_planes" and Cout % 8 == 0:
            grads = []
            y.register_hook(grads.append)               # the gradient object _Conv.backward receives
            _norm_act(row, y).backward(_nhwc(B, Cout, Hs, Hs, gen))
            dy = grads[0]
            assert getattr(dy, "_vp_split", None) is not None, "the normalisation's input gradient must carry split planes"
        else:
            dy = _nhwc(B, Cout, Hs, Hs, gen)
            y.backward(dy)
        torch.cuda.synchronize()
        report = []
        _families(report, tau_mode, x.detach(), dy.detach(), w.detach(), stride, y.detach(), x.grad, w.grad, seed,
                  bias=None if b is None else b.detach())
        if b is not None:
            _check(report, "dbias", "f32", b.grad[None], dy.double().sum((0, 2, 3))[None], dy.double().abs().sum((0, 2, 3))[None],
                   torch.full((1, Cout), B * Hs * Hs, device=DEV))
        print(f"direct-sum err/tau {row} {layer} {mode} {feed}: " + ", ".join(report))
    finally:
        FH.set_conv_precision(prev)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("H,W,stride", [(7, 9, 2), (7, 7, 1)], ids=["7x9-s2", "7x7-s1"])
def test_conv5x5_on_an_odd_image_matches_the_direct_sum(H, W, stride, mode):
    """functional.conv5x5, 8 -> 16 channels, on an image with odd sides: the output is floor((n + 4 - 5) / stride) + 1 wide, so with
    stride 2 the big side is not twice the small one; y, dx and dW against the direct sums"""
    from vae_play_amd import functional as FH
    B, Cin, Cout = 2, 8, 16
    seed = 97 * H + 13 * W + stride
    gen = torch.Generator(device=DEV).manual_seed(seed)
    prev = FH.get_conv_precision()
    FH.set_conv_precision(mode)
    try:
        x = _nhwc(B, Cin, H, W, gen).requires_grad_(True)
        w = (torch.randn(Cout, Cin, 5, 5, device=DEV, generator=gen) * (2.0 / (Cin * 25)) ** 0.5).requires_grad_(True)
        y = FH.conv5x5(x, w, None, stride, None)
        Hs, Ws = R.out_size(H, 5, stride), R.out_size(W, 5, stride)
        assert tuple(y.shape) == (B, Cout, Hs, Ws)
        dy = _nhwc(B, Cout, Hs, Ws, gen)
        y.backward(dy)
        torch.cuda.synchronize()
        assert tuple(x.grad.shape) == (B, Cin, H, W)
        report = []
        _families(report, mode, x.detach(), dy, w.detach(), stride, y.detach(), x.grad, w.grad, seed)
        print(f"direct-sum err/tau conv5x5 {H}x{W} stride {stride} {mode}: " + ", ".join(report))
    finally:
        FH.set_conv_precision(prev)


def _record_conv_shapes(monkeypatch):
    """(entry point, B, Cin, Cout, ks, stride, H, W) of every functional.conv2d / conv5x5 launch from now on"""
    from vae_play_amd import functional as FH
    seen = set()
    o2, o5 = FH.conv2d, FH.conv5x5

    def rec2(x, weight, bias=None, stride=1):
        seen.add(("conv2d", x.shape[0], weight.shape[1], weight.shape[0], weight.shape[2], stride, x.shape[2], x.shape[3]))
        return o2(x, weight, bias, stride)

    def rec5(x, weight, bias=None, stride=2, act=None):
        seen.add(("conv5x5", x.shape[0], weight.shape[1], weight.shape[0], 5, stride, x.shape[2], x.shape[3]))
        return o5(x, weight, bias, stride, act)

    monkeypatch.setattr(FH, "conv2d", rec2)
    monkeypatch.setattr(FH, "conv5x5", rec5)
    return seen


@pytest.mark.parametrize("row", ["be_heads", "be_gan", "font", "vaegan"])
def test_front_end_table_covers_every_model_convolution(row, monkeypatch):
    """one forward of the row's models at the bench shape with both conv entry points recorded: every distinct
    (entry, B, Cin, Cout, ks, stride, H, W) it launches is in FRONT, so a layer added later cannot escape the direct-sum test"""
    from vae_play_amd import networks as V, networks_BE as N, networks_BE_GAN as NG, networks_BE_font as NF
    seen = _record_conv_shapes(monkeypatch)
    g = torch.Generator(device=DEV).manual_seed(0)
    img = 256
    with torch.no_grad(), torch.device(DEV):          # (parameters initialised on the device: the font model's dense layers are large)
        if row == "be_heads":
            net = N.ComposeNet(N.FeatureNet(None, in_channels=256, target_out_channels=32)).to(DEV).train()
            net(torch.randn(16, 256, img // 4, img // 4, device=DEV, generator=g))
        elif row == "be_gan":
            G = NG.ComposeNet(3, img, feature_channels=256).to(DEV).train()
            D = NG.Discriminator(3, img, 5).to(DEV).train()
            G(torch.randn(16, 256, img // 4, img // 4, device=DEV, generator=g))
            m = (torch.rand(16, 1, img, img, device=DEV, generator=g) > 0.5).float()
            D(torch.rand(16, 3, img, img, device=DEV, generator=g), m, m)
        elif row == "font":
            B = 8
            net = NF.ComposeNet(img).to(DEV).train()
            disc = NF.Discriminator(img, 2, 143).to(DEV).train()
            x = torch.rand(B, 3, img, img, device=DEV, generator=g)
            cls = torch.zeros(B, 143, device=DEV)
            cls[torch.arange(B), torch.arange(B)] = 1
            y = {"cls": cls, "cnt_style": torch.rand(B, 5, device=DEV, generator=g)}
            pr = net(x, y)                                 # generator phase
            net(x)                                         # style-encoder phase
            disc(torch.cat([pr["masks"], pr["edges"]], dim=1), y)
        else:
            net = V.VaeGan(128, 128).to(DEV).train()
            net(torch.rand(16, 1, 128, 128, device=DEV, generator=g))
    table = {(_entry(l[0]), l[7], l[2], l[3], l[4], l[5], l[6], l[6]) for l in FRONT if l[0] == row}
    assert seen, "no convolution recorded"
    missing = sorted(seen - table)
    assert not missing, f"{row}: convolutions launched but not in the direct-sum table (entry, B, Cin, Cout, ks, stride, H, W): {missing}"


# ---- b. the C ABI at shapes that run each internal path ---------------------------------------------------------------------------------
# (id naming the path(s), mode, B, Cb, Cs, Hb, Wb, ks, stride); Hs = floor((Hb + 2p - ks) / s) + 1
ABI = [("f32-narrow_gather-narrow_wgrad_small_side", "f32", 4, 64, 3, 64, 64, 5, 1),
       ("f32-igemm_k5s2_cb3-narrow_wgrad_big_side", "f32", 4, 3, 32, 64, 64, 5, 2),
       ("f32-fast_gather-fast_scatter-wgrad5_rows", "f32", 4, 64, 128, 32, 32, 5, 2),
       ("f32-igemm_k5s2_odd_hb-splitk_wgrad", "f32", 4, 32, 64, 31, 31, 5, 2),
       ("f32-igemm_k3s2_odd_hb-splitk_slab_reduce_v4", "f32", 8, 64, 64, 33, 33, 3, 2),
       ("f32-igemm_k3s1_nonsquare-tiny_weight_deep_split", "f32", 4, 8, 8, 40, 56, 3, 1),
       ("f32-igemm_k1s2_odd_hb", "f32", 4, 16, 32, 31, 31, 1, 2),
       ("bf16x3-igemm16_k3s2_odd_hb-tap_pairs_64x64", "bf16x3", 4, 32, 64, 33, 33, 3, 2),
       ("bf16x3-igemm16_k3s1-tap_pairs_128x128", "bf16x3", 2, 64, 128, 32, 32, 3, 1),
       ("bf16x3-igemm16_k3s2_odd_hb-tap_pairs_64x128", "bf16x3", 4, 64, 64, 31, 31, 3, 2),
       ("bf16x3-igemm16_k1s1-wide_64x128", "bf16x3", 4, 128, 64, 32, 32, 1, 1),
       ("bf16x3-igemm16_k1s2_odd_hb-splitk_wgrad", "bf16x3", 4, 16, 32, 31, 31, 1, 2),
       ("bf16x3-igemm16_k5s2_odd_hb-splitk_wgrad", "bf16x3", 2, 16, 24, 33, 33, 5, 2),
       ("bf16x3-halo_gather_k5s1-splitk_wgrad", "bf16x3", 2, 32, 32, 32, 32, 5, 1),
       ("bf16x3-halo_scatter_k5s1_cs8", "bf16x3", 2, 16, 8, 32, 32, 5, 1),
       ("bf16x3-halo_gather_k5s2_cb8", "bf16x3", 2, 8, 16, 32, 32, 5, 2)]


@pytest.mark.parametrize("name,mode,B,Cb,Cs,Hb,Wb,ks,stride", ABI, ids=[a[0] for a in ABI])
def test_c_abi_path_matches_the_direct_sum(name, mode, B, Cb, Cs, Hb, Wb, ks, stride):
    from vae_play_amd import ops
    seed = sum(map(ord, name))
    gen = torch.Generator(device=DEV).manual_seed(seed)
    Hs, Ws = R.out_size(Hb, ks, stride), R.out_size(Wb, ks, stride)
    x, y = _nhwc(B, Cb, Hb, Wb, gen), _nhwc(B, Cs, Hs, Ws, gen)
    w = torch.randn(Cs, Cb, ks, ks, device=DEV, generator=gen) * 0.05
    if mode == "f32":
        p0, p1 = ops.pack_w(w, True, True)
        gather = ops.conv_gather(x, p0, None, ks, stride)
        scatter = ops.conv_scatter(y, p1, ks, stride, Hb, Wb)
        dw = ops.conv_wgrad(x, y, ks, stride)
    else:
        p0, p1 = ops.pack_w_split(w, True, True)
        xs, ys = ops.split_f32(x), ops.split_f32(y)
        gather = ops.conv_gather_bf16x3(xs, tuple(x.shape), p0, Cs, None, ks, stride)
        scatter = ops.conv_scatter_bf16x3(ys, tuple(y.shape), p1, Cb, ks, stride, Hb, Wb)
        dw = ops.conv_wgrad_bf16x3(xs, tuple(x.shape), ys, tuple(y.shape), ks, stride)
    assert tuple(gather.shape) == (B, Cs, Hs, Ws) and tuple(scatter.shape) == (B, Cb, Hb, Wb)
    report = []
    _families(report, mode, x, y, w, stride, gather, scatter, dw, seed)
    print(f"direct-sum err/tau C ABI {name}: " + ", ".join(report))


# ---- c. the fused steps' first layer: im2col + 1x1 layer, weight gradient unpacked from the im2col column order ---------------------------
GSCALE = 16.0     # power-of-two scale of the gradient operand of the two-product launches (undone by out_scale)


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x2"])
def test_first_layer_im2col_matches_the_5x5_direct_sum(mode):
    """B = 32, 128 px, 3 image channels (NCHW, as the fused steps read the batch), 64 outputs: the 5x5 stride-2 gather through
    vp_im2col5s2_* + the ks = 1 gather, the weight gradient through the ks = 1 weight gradient + vp_unpack_dw_im2col5_f32"""
    from vae_play_amd import _lib, ops
    lib = _lib.load()
    B, Cb, Cs, Hb = 32, 3, 64, 128
    Hs = Hb // 2
    gen = torch.Generator(device=DEV).manual_seed(1234)
    x = torch.randn(B, Cb, Hb, Hb, device=DEV, generator=gen)            # NCHW
    dy = _nhwc(B, Cs, Hs, Hs, gen)
    w = torch.randn(Cs, Cb, 5, 5, device=DEV, generator=gen) * 0.05
    KC = lib.vp_im2col5s2_cols(Cb)
    npix = B * Hs * Hs
    S = ops._stream()
    dwc = torch.empty(Cs, KC, device=DEV)
    dw = torch.empty(Cs, Cb, 5, 5, device=DEV)
    outs = []         # (family, tau mode, result, reference weight, reference big side)
    if mode == "f32":
        xcol = torch.empty(npix * KC, device=DEV)
        w0 = torch.empty(Cs * KC, device=DEV)
        _lib.call("vp_im2col5s2_f32", ops._p(x), ops._p(xcol), B, Cb, Hb, Hb, 1, S)
        _lib.call("vp_pack_w_im2col5_f32", ops._p(w), ops._p(w0), Cs, Cb, S)
        xc = xcol.view(B, Hs, Hs, KC).permute(0, 3, 1, 2)
        g = ops.conv_gather(xc, w0.view(Cs, 1, KC), None, 1, 1)
        ops.conv_wgrad(xc, dy, 1, 1, out=dwc.view(Cs, KC, 1, 1))
        _lib.call("vp_unpack_dw_im2col5_f32", ops._p(dwc), ops._p(dw), Cs, Cb, S)
        outs += [("gather", "f32", g, w, x), ("wgrad", "f32", dw, w, x)]
    else:
        fmt = ops.SPLIT_BF16 if mode == "bf16x3" else ops.SPLIT_F16
        xcol = ops.empty_split(npix * KC, x)
        w0s = ops.empty_split(Cs * KC, x)
        _lib.call("vp_im2col5s2_split_fmt_f32", ops._p(x), ops._pv(xcol), B, Cb, Hb, Hb, 1, fmt, S)
        _lib.call("vp_pack_w_im2col5_split_fmt", ops._p(w), ops._pv(w0s), Cs, Cb, fmt, S)
        ws = ops._ws(lib.vp_conv_wgrad_bf16x3_workspace_bytes(B, Hs, Hs, Hs, Hs, KC, Cs, 1, 1), x)
        geom = (B, Hs, Hs, Hs, Hs, KC, Cs, 1, 1)
        if mode == "bf16x3":
            g = ops.empty_cl(B, Cs, Hs, Hs, x)
            _lib.call("vp_conv_gather_bf16x3", ops._pv(xcol), ops._pv(w0s), None, ops._p(g), *geom, 0, S)
            _lib.call("vp_conv_wgrad_bf16x3", ops._pv(xcol), ops._pv(ops.split_f32(dy)), ops._p(dwc), *geom, ops._p(ws), ws.numel() * 4, S)
            _lib.call("vp_unpack_dw_im2col5_f32", ops._p(dwc), ops._p(dw), Cs, Cb, S)
            outs += [("gather", "bf16x3", g, w, x), ("wgrad", "bf16x3", dw, w, x)]
        else:
            for products in (3, 2):
                g = ops.empty_cl(B, Cs, Hs, Hs, x)
                _lib.call("vp_conv_gather_f16", ops._pv(xcol), ops._pv(w0s), None, ops._p(g), *geom, 0, products, 1.0, S)
                outs.append(("gather", f"f16x2/{products}", g, w, x))
            # the weight gradient of the fused step: two products, the gradient planes scaled by GSCALE; x keeps its hi plane only
            _lib.call("vp_conv_wgrad_f16x2", ops._pv(xcol), ops._pv(ops.split_f32(dy, fmt, GSCALE)), ops._p(dwc), *geom, 1.0 / GSCALE,
                      ops._p(ws), ws.numel() * 4, S)
            _lib.call("vp_unpack_dw_im2col5_f32", ops._p(dwc), ops._p(dw), Cs, Cb, S)
            outs += [("wgrad", "f16x2/2", dw, w, x), ("wgrad", "f16x2/2 declared", dw, w, x.half().float())]
    torch.cuda.synchronize()
    gp = R.gather_points(B, Hs, 7)
    cs, cb = R.tile_channels(Cs), list(range(Cb))
    report = []
    for family, key, got, wr, xr in outs:
        if family == "gather":
            _check(report, family, key, R.take(got, gp), *R.gather_ref(xr, wr, gp, terms=True))
        else:
            _check(report, family, key, got[cs][:, cb], *R.wgrad_ref(xr, dy, cs, cb, terms=True))
    print(f"direct-sum err/tau first layer im2col {mode}: " + ", ".join(report))
