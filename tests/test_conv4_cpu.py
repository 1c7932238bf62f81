"""4x4 convolutions (kernel 4, padding 1: the Style-GAN generator's, models/network_Style_GAN.py:49,95-98,116) without a GPU:
the index math of the three families through the host emulation (tests/host_emul/emul.cpp compiles csrc/problems.h) against torch,
and the drop-in boundary of blocks.Conv2d(.., 4, 2), network_Style_GAN.ConvTranspose2d and StyleUp.

An even kernel makes the scatter family's phase grid ceil(Hb / s) x ceil(Wb / s) larger than the small image when the big side is
odd or the stride is 1 (Hs = floor(Hb / 2) at stride 2, Hb - 1 at stride 1): the outputs are pre-filled with NaN so that a pixel the
kernel never writes shows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_index_math import close, emul, nhwc, ptr  # noqa: F401  (emul: the module-scoped fixture that builds the library)
from tests.util import load_golden, t

# (B, Cb, Cs, Hb, Wb, stride)
CASES = [(2, 8, 16, 8, 8, 2), (2, 4, 8, 6, 10, 2), (3, 3, 8, 7, 9, 2), (2, 8, 4, 7, 9, 1), (1, 64, 32, 4, 4, 2)]
KS, PAD = 4, 1


def _layer(B, Cb, Cs, Hb, Wb, stride, seed):
    g = torch.Generator().manual_seed(seed)
    Hs, Ws = (Hb + 2 * PAD - KS) // stride + 1, (Wb + 2 * PAD - KS) // stride + 1
    big = torch.randn(B, Cb, Hb, Wb, generator=g)
    w = torch.randn(Cs, Cb, KS, KS, generator=g)
    bias = torch.randn(Cs, generator=g)
    gy = torch.randn(B, Cs, Hs, Ws, generator=g)
    return big, w, bias, gy, Hs, Ws


@pytest.mark.parametrize("B,Cb,Cs,Hb,Wb,stride", CASES)
def test_gather_k4_is_conv2d(emul, B, Cb, Cs, Hb, Wb, stride):
    big, w, bias, _, Hs, Ws = _layer(B, Cb, Cs, Hb, Wb, stride, 11)
    ref = F.conv2d(big, w, bias, stride=stride, padding=PAD)
    assert tuple(ref.shape[2:]) == (Hs, Ws)
    out = torch.full((B, Hs, Ws, Cs), float("nan"))
    emul.emul_conv_gather(ptr(nhwc(big)), ptr(w.permute(0, 2, 3, 1).contiguous()), ptr(bias), ptr(out), B, Hs, Ws, Hb, Wb, Cb, Cs, KS,
                          stride, 0)
    assert not torch.isnan(out).any()
    close(out, nhwc(ref))


@pytest.mark.parametrize("B,Cb,Cs,Hb,Wb,stride", CASES)
def test_scatter_k4_writes_every_pixel_and_is_the_input_gradient(emul, B, Cb, Cs, Hb, Wb, stride):
    big, w, _, gy, Hs, Ws = _layer(B, Cb, Cs, Hb, Wb, stride, 12)
    bigr = big.clone().requires_grad_(True)
    F.conv2d(bigr, w, None, stride=stride, padding=PAD).backward(gy)
    out = torch.full((B, Hb, Wb, Cb), float("nan"))
    emul.emul_conv_scatter(ptr(nhwc(gy)), ptr(w.permute(1, 2, 3, 0).contiguous()), ptr(out), B, Hs, Ws, Hb, Wb, Cs, Cb, KS, stride)
    assert not torch.isnan(out).any(), "some pixels of the big side were never written"
    close(out, nhwc(bigr.grad))
    if stride == 2 and Hb == 2 * Hs and Wb == 2 * Ws:      # the same launch is nn.ConvTranspose2d(Cs, Cb, 4, 2, 1)'s forward
        close(out, nhwc(F.conv_transpose2d(gy, w, None, stride=2, padding=1)))


@pytest.mark.parametrize("B,Cb,Cs,Hb,Wb,stride", CASES)
@pytest.mark.parametrize("split", [0, 3])
def test_wgrad_k4_is_autograd(emul, B, Cb, Cs, Hb, Wb, stride, split):
    big, w, _, gy, Hs, Ws = _layer(B, Cb, Cs, Hb, Wb, stride, 13)
    wr = w.clone().requires_grad_(True)
    F.conv2d(big, wr, None, stride=stride, padding=PAD).backward(gy)
    dw = torch.full((Cs, Cb, KS, KS), float("nan"))
    emul.emul_conv_wgrad(ptr(nhwc(big)), ptr(nhwc(gy)), ptr(dw), B, Hs, Ws, Hb, Wb, Cb, Cs, KS, stride, split)
    close(dw, wr.grad)


# ---- the drop-in boundary ------------------------------------------------------------------------------------------------
def test_blocks_conv2d_accepts_kernel_4():
    from vae_play_amd import blocks
    m = blocks.Conv2d(8, 16, 4, 2, bn="instance")
    g = load_golden("stylegan_conv2d_k4s2_instance_relu")
    keys = sorted(k[len("param/"):] for k in g if k.startswith("param/"))
    assert sorted(m.state_dict()) == keys == ["conv.0.weight"]
    assert tuple(m.state_dict()["conv.0.weight"].shape) == (16, 8, 4, 4)
    torch.manual_seed(int(g["seed"]))
    m = blocks.Conv2d(8, 16, 4, 2, bn="instance")
    assert np.array_equal(m.state_dict()["conv.0.weight"].numpy(), g["param/conv.0.weight"])
    for ks in (2, 6, 7):
        with pytest.raises(ValueError):
            blocks.Conv2d(8, 16, ks, 2)


def test_conv_transpose2d_init_equals_torch():
    from vae_play_amd.network_Style_GAN import ConvTranspose2d
    torch.manual_seed(3)
    ours = ConvTranspose2d(16, 8, 4, 2, 1)
    torch.manual_seed(3)
    ref = torch.nn.ConvTranspose2d(16, 8, 4, 2, 1)
    assert list(ours.state_dict()) == list(ref.state_dict()) == ["weight", "bias"]
    for k, v in ref.state_dict().items():
        assert torch.equal(ours.state_dict()[k], v), k
    g = load_golden("stylegan_convt_k4s2")
    torch.manual_seed(int(g["seed"]))
    ours = ConvTranspose2d(16, 8, 4, 2, 1)
    for k, v in ours.state_dict().items():
        assert np.array_equal(v.numpy(), g["param/" + k]), k
    assert ConvTranspose2d(16, 8, 4, 2, 1, bias=False).bias is None


def test_styleup_keys_and_seeded_init_equal_the_fixture():
    from vae_play_amd.network_Style_GAN import StyleUp
    g = load_golden("stylegan_up_16to8")
    ref = {k[len("param/"):]: v for k, v in g.items() if k.startswith("param/")}
    torch.manual_seed(int(g["seed"]))
    sd = StyleUp(16, 8).state_dict()
    assert list(sd) == (["up_convs.0.weight", "up_convs.0.bias", "cat_convs.0.conv.0.weight", "cat_convs.0.conv.0.bias"]
                        + [f"cat_convs.{i}.{m}.{p}" for i in (1, 2) for m in ("cSE.1", "cSE.3", "sSE.0") for p in ("weight", "bias")])
    assert sorted(sd) == sorted(ref) and len(sd) == 16
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), ref[k]), k


def test_style_gan_alias_resolves():
    import models.network_Style_GAN as alias
    import vae_play_amd.network_Style_GAN as impl
    assert alias.StyleUp is impl.StyleUp and alias.ConvTranspose2d is impl.ConvTranspose2d


def test_cpu_tensors_raise():
    from vae_play_amd import _lib, blocks, functional as FH
    from vae_play_amd.network_Style_GAN import ConvTranspose2d, StyleUp
    with pytest.raises(_lib.VaePlayHipError):
        ConvTranspose2d(16, 8, 4, 2, 1)(torch.randn(1, 16, 4, 4))
    with pytest.raises(_lib.VaePlayHipError):
        FH.conv_transpose2d(torch.randn(1, 3, 4, 4), torch.randn(3, 5, 4, 4))
    with pytest.raises(_lib.VaePlayHipError):
        blocks.Conv2d(8, 16, 4, 2, bn="instance")(torch.randn(1, 8, 8, 8))
    with pytest.raises(_lib.VaePlayHipError):
        StyleUp(16, 8)(torch.randn(1, 16, 4, 4), torch.randn(1, 8, 8, 8))


@pytest.mark.parametrize("k,s,p", [(5, 2, 2), (4, 1, 1), (4, 2, 0), (3, 2, 1), (4, 2, 2)])
def test_unsupported_transposed_geometry_raises(k, s, p):
    from vae_play_amd import functional as FH
    from vae_play_amd.network_Style_GAN import ConvTranspose2d
    with pytest.raises(ValueError):
        ConvTranspose2d(16, 8, k, s, p)
    if (k, s) != (4, 2):
        with pytest.raises(ValueError):
            FH.conv_transpose2d(torch.randn(1, 16, 4, 4), torch.randn(16, 8, k, k), None, s)
