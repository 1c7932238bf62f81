"""The convolution launches that StyleEncoder and Discriminator (models/network_Style_GAN.py:12-43, :201-229) add to the ones the
other networks run, through the autograd front end functional.conv2d in both arithmetic modes: forward, input gradient, weight
gradient and bias gradient against the fp64 direct sums of tests/conv_ref.py, |out - r| <= tau(K, mode) * A with conv_ref's tau, as
tests/test_gpu_conv4.py holds its layers -- no tolerance of its own.  Every test prints its figures before it asserts."""
import pytest
import torch

from tests import conv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, Cin, Cout, H, W, ks, stride)
LAYERS = {"enc_first_3to64_k5": (2, 3, 64, 16, 16, 5, 1),        # StyleEncoder.convs.0
          "disc_first_6to64_k5": (2, 6, 64, 16, 16, 5, 1),       # Discriminator.convs.0: image and content image side by side
          "k3s2_32to32_4to2": (2, 32, 32, 4, 4, 3, 2),           # convs.3 of the encoder, adv_convs.0 / aux_convs.0
          "k3s2_32to32_2to1": (2, 32, 32, 2, 2, 3, 2),           # convs.4 of the encoder: one output pixel, four live taps
          "k3s2_32to1_2to1": (2, 32, 1, 2, 2, 3, 2),             # adv_convs.1 on the composed path
          "k3s2_32to3_2to1": (2, 32, 3, 2, 2, 3, 2)}             # aux_convs.1 on the composed path


class _precision:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from vae_play_amd import functional as FH
        self.prev = FH.get_conv_precision()
        FH.set_conv_precision(self.mode)

    def __exit__(self, *a):
        from vae_play_amd import functional as FH
        FH.set_conv_precision(self.prev)


def _nhwc(B, C, H, W, gen):
    return torch.randn(B, H, W, C, device=DEV, generator=gen).permute(0, 3, 1, 2)


def _check(label, mode, got, r, A, K):
    assert not torch.isnan(got).any(), f"{label} {mode}: sampled outputs that the kernel never wrote"
    ratio, i, err = R.worst_scaled(got, r, A, R.tau(K, mode).to(r.device))
    print(f"  {label}[{mode}] worst err/tau {ratio:.3f} (|out - r| = {err:.2e} * A, K = {int(K.flatten()[i])})")
    assert ratio <= 1.0, f"{label} {mode}: |out - r| = {err:.2e} * A at flat sample {i} exceeds tau(K = {int(K.flatten()[i])})"


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("layer", list(LAYERS))
def test_functional_conv2d_at_the_networks_launch_shapes(layer, mode):
    from vae_play_amd import functional as FH
    B, Cin, Cout, H, W, ks, stride = LAYERS[layer]
    seed = sum(LAYERS[layer])
    gen = torch.Generator(device=DEV).manual_seed(seed)
    with _precision(mode):
        x = _nhwc(B, Cin, H, W, gen).requires_grad_(True)
        w = (torch.randn(Cout, Cin, ks, ks, device=DEV, generator=gen) * (2.0 / (Cin * ks * ks)) ** 0.5).requires_grad_(True)
        b = (torch.randn(Cout, device=DEV, generator=gen) * 0.1).requires_grad_(True)
        y = FH.conv2d(x, w, b, stride)
        Hs, Ws = R.out_size(H, ks, stride), R.out_size(W, ks, stride)
        assert tuple(y.shape) == (B, Cout, Hs, Ws)
        dy = _nhwc(B, Cout, Hs, Ws, gen)
        y.backward(dy)
        torch.cuda.synchronize()
    print(f"direct-sum err/tau functional.conv2d {layer} {LAYERS[layer]} {mode}:")
    xd, wd, bd = x.detach(), w.detach(), b.detach()
    gp = R.gather_points(B, Hs, seed, Ws=Ws)
    r, A, K = R.gather_ref(xd, wd, gp, stride, terms=True)
    _check("forward", mode, R.take(y.detach(), gp), r + bd.double(), A + bd.double().abs(), K + 1)
    assert not torch.isnan(x.grad).any(), f"input gradient {mode}: pixels never written"
    sp = R.scatter_points(B, H, seed, Wb=W)
    _check("input gradient", mode, R.take(x.grad, sp), *R.scatter_ref(dy, wd, sp, stride, terms=True))
    cs, cb = R.tile_channels(Cout), R.tile_channels(Cin)
    _check("weight gradient", mode, w.grad[cs][:, cb], *R.wgrad_ref(xd, dy, cs, cb, ks, stride, terms=True))
    _check("bias gradient", "f32", b.grad[None], dy.double().sum((0, 2, 3))[None], dy.double().abs().sum((0, 2, 3))[None],
           torch.full((1, Cout), B * Hs * Ws, device=DEV))
