"""Drop-in classes for kungyao/vae-play's ``models/network_Style_GAN.py`` on the HIP back end: the Style-GAN generator and the
blocks it is made of, the style encoder and the discriminator.

Same constructor signatures and ``state_dict`` keys as the reference:
  ConvTranspose2d(in, out, 4, 2, 1)  nn.ConvTranspose2d with its default bias                    models/network_Style_GAN.py:49,116
     keys weight (in, out, 4, 4), bias (out); the bias is added in the scatter kernel's epilogue
  StyleUp(in_channel, out_channel)                                                               models/network_Style_GAN.py:45-65
     keys up_convs.0.{weight,bias}, cat_convs.0.conv.0.{weight,bias}, cat_convs.{1,2}.{cSE.1,cSE.3,sSE.0}.{weight,bias}
  myConv2d(in, out, k, stride=1, bn=None, activate='relu')   conv_1(x) * (1 - label) + conv_2(x) * label      :72-79
     keys conv_{1,2}.conv.0.weight[, bias]; one convolution with the two weights stacked along the output channel, then one
     normalise-and-blend pass (functional.pair_blend); ``_PAIR_FUSED = False`` or a case the fused form does not cover
     (bn="batch", a label that is not one number per image, a label that requires grad) runs the reference's expression
  MLP(nf_in, nf_out, num_blocks)     keys model.{i}.fc.0.{weight,bias}, the reference's width rule                   :182-199
  Generator(image_size, z_dim, max_channels=256)   encode / decode / forward(x, style_code, labels), 81 keys         :81-180
  StyleEncoder(z_dim, image_size, max_channels=1024)   forward(x) -> (mu, logvar)                                    :12-43
     keys convs.0.conv.0.{weight,bias} (5x5), convs.{1..n}.conv.0.weight (3x3 stride 2 + InstanceNorm), two more stride-2 convs
     with bias, fc_{mu,logvar}.fc.0.{weight,bias}
  Discriminator(image_size, num_of_classes, max_channels=256)   forward(x, x_content, y) -> (adv_res, aux_res)       :201-229
     keys convs.*, adv_convs.{0,1}.conv.0.{weight,bias}, aux_convs.{0,1}.conv.0.{weight,bias}; the two last convolutions with
     their sigmoid and softmax run as one kernel (functional.twin_head) when they see 2 x 2 maps; ``_HEAD_FUSED = False`` or a
     case the kernel does not cover runs the reference's expression
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import functional as F_hip
from .blocks import _CONV_LRELU, Conv2d, Linear, SCSEBlock, _NoParams, _act_name

IMAGE_CHANNEL = 3
_HEAD_FUSED = True           # Discriminator's output stage as functional.twin_head; False: the reference's expression (A/B runs)
_HEAD_MAX_C, _HEAD_MAX_K = 1024, 64      # the range of vp_twin_head_*_f32 (include/vaeplay_hip.h)
_PAIR_FUSED = True           # myConv2d as one stacked convolution + functional.pair_blend; False: the reference's expression (A/B runs)


class ConvTranspose2d(nn.Module):
    """nn.ConvTranspose2d's weight/bias layout, key names and default init; kernel 4, stride 2, padding 1 only."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stride: int = 1, padding: int = 0, bias: bool = True):
        super().__init__()
        if (kernel_size, stride, padding) != (4, 2, 1):
            raise ValueError("HIP ConvTranspose2d supports kernel_size 4, stride 2, padding 1")
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels, 4, 4))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in, _ = nn.init._calculate_fan_in_and_fan_out(self.weight)
            if fan_in != 0:
                bound = 1 / math.sqrt(fan_in)
                nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        return F_hip.conv_transpose2d(x, self.weight, self.bias, 2)


class StyleUp(nn.Module):
    """models/network_Style_GAN.py:45-65: transposed conv + InstanceNorm + ReLU, concatenation with the skip tensor, Conv2d(3) + ReLU,
    two SCSEBlocks and a final ReLU (fused into the second block's store).  Parameters are created in the reference's order, so the
    seeded default init equals its."""

    def __init__(self, in_channel, out_channel):
        super().__init__()
        self.up_convs = nn.Sequential(ConvTranspose2d(in_channel, out_channel, 4, 2, 1), _NoParams(), _NoParams())
        self.cat_convs = nn.Sequential(Conv2d(out_channel * 2, out_channel, 3), SCSEBlock(out_channel, reduction=4),
                                       SCSEBlock(out_channel, reduction=4), _NoParams())

    def forward(self, x, skip):
        x = self.up_convs[0](x)
        x = F_hip.instance_norm_act(x, 1e-5, "relu")
        x = torch.cat([x, skip], dim=1)
        x = self.cat_convs[0](x)
        x = self.cat_convs[1](x)
        return self.cat_convs[2](x, relu=True)


class myConv2d(nn.Module):
    """models/network_Style_GAN.py:72-79: two independent Conv2d blocks on the same input, blended per image by ``label``.  The
    blocks are held as ``conv_1`` / ``conv_2`` (the reference's keys and seeded init); the fused forward reads their parameters."""

    def __init__(self, in_channel, out_channel, kernel_size, stride=1, bn=None, activate='relu'):
        super().__init__()
        self.conv_1 = Conv2d(in_channel, out_channel, kernel_size, stride, bn, activate)
        self.conv_2 = Conv2d(in_channel, out_channel, kernel_size, stride, bn, activate)
        self.stride, self.bn, self.act = stride, bn, _act_name(activate)

    def uses_fused(self, x, label) -> bool:
        """Does forward(x, label) take the stacked convolution + pair_blend?  One label per image (shape (B,) or (B, 1, ..., 1)),
        no gradient asked for the label, bn None or "instance", and the module-level switch on."""
        B = x.shape[0]
        per_image = label.dim() >= 1 and label.shape[0] == B and label.numel() == B
        return bool(_PAIR_FUSED and self.bn in (None, "instance") and per_image and not label.requires_grad)

    def forward(self, x, label):
        if not self.uses_fused(x, label):
            return self.conv_1(x) * (1 - label) + self.conv_2(x) * label
        p1, p2 = self.conv_1.conv[0], self.conv_2.conv[0]
        bias = None if p1.bias is None else torch.cat([p1.bias, p2.bias])
        u = F_hip.conv2d(x, torch.cat([p1.weight, p2.weight]), bias, self.stride)
        return F_hip.pair_blend(u, label, self.bn == "instance", 1e-5, self.act, _CONV_LRELU)


class MLP(nn.Module):
    """models/network_Style_GAN.py:182-199: ``num_blocks`` Linear layers without activation, widths nf_in -> nf_in -> ... -> nf_out
    growing by the reference's integer ratio."""

    def __init__(self, nf_in, nf_out, num_blocks):
        super().__init__()
        self.model = nn.Sequential(*[Linear(i, o, activate=None) for i, o in self.widths(nf_in, nf_out, num_blocks)])

    @staticmethod
    def widths(nf_in, nf_out, num_blocks):
        """(in, out) of every layer by the reference's rule, its truncations included"""
        dims = [(nf_in, nf_in)]
        out_dim = nf_in
        ratio = int(2 ** (int(math.log2(nf_out / nf_in)) / (num_blocks - 1)))
        for _ in range(num_blocks - 2):
            in_dim = out_dim
            out_dim = min(in_dim * ratio, nf_out)
            dims.append((in_dim, out_dim))
        dims.append((out_dim, nf_out))
        return dims

    def forward(self, x):
        return self.model(x.reshape(x.size(0), -1))


class Generator(nn.Module):
    """models/network_Style_GAN.py:81-180: the style code becomes a fourth image channel through ``mlp``; six label-gated
    convolutions encode, three StyleUp blocks decode against Conv2d(3) + InstanceNorm skips, ``final`` ends in tanh.  Modules are
    created in the reference's order, so keys, their order and the seeded default init equal its."""

    def __init__(self, image_size, z_dim, max_channels=256):
        super().__init__()
        self.z_dim = z_dim
        self.image_size = image_size
        self.conv1 = myConv2d(IMAGE_CHANNEL + 1, 32, 3, 1, activate=None)
        self.conv2 = myConv2d(32, 32, 3, 1, activate=None)
        self.down1 = myConv2d(32, 64, 4, 2, bn="instance")
        self.down2 = myConv2d(64, 128, 4, 2, bn="instance")
        self.down3 = myConv2d(128, 256, 4, 2, bn="instance")
        self.down4 = myConv2d(256, 256, 4, 2, bn="instance")
        self.up1 = StyleUp(256, 256)
        self.up2 = StyleUp(256, 128)
        self.up3 = StyleUp(128, 64)
        self.skip1 = Conv2d(256, 256, 3, 1, bn="instance")
        self.skip2 = Conv2d(128, 128, 3, 1, bn="instance")
        self.skip3 = Conv2d(64, 64, 3, 1, bn="instance")
        self.final = nn.Sequential(ConvTranspose2d(64, 32, 4, 2, 1), Conv2d(32, 32, 3, 1, bn=None), Conv2d(32, 32, 3, 1, bn=None),
                                   Conv2d(32, IMAGE_CHANNEL, 3, 1, bn=None, activate=None), _NoParams())
        self.mlp = MLP(z_dim, image_size * image_size, 3)

    def encode(self, x, style_code, labels):
        style_code = self.mlp(style_code)
        style_code = style_code.reshape(style_code.size(0), 1, self.image_size, self.image_size)
        x = torch.cat([x, style_code], dim=1)
        labels = labels.reshape(labels.size(0), 1, 1, 1)
        x = self.conv2(self.conv1(x, labels), labels)
        d1 = self.down1(x, labels)
        d2 = self.down2(d1, labels)
        d3 = self.down3(d2, labels)
        d4 = self.down4(d3, labels)
        return x, d1, d2, d3, d4

    def decode(self, c0, d1, d2, d3, d4, style_code):
        up1 = self.up1(d4, self.skip1(d3))
        up2 = self.up2(up1, self.skip2(d2))
        up3 = self.up3(up2, self.skip3(d1))
        x = up3
        for m in list(self.final)[:4]:
            x = m(x)
        return F_hip.activation(x, "tanh")

    def forward(self, x, style_code, labels):
        c0, d1, d2, d3, d4 = self.encode(x, style_code, labels)
        return self.decode(c0, d1, d2, d3, d4, style_code)


def _n_level(image_size):
    return int(math.log2(image_size)) - 2


def _flatten(x):
    """``x.reshape(x.size(0), -1)`` of the logical NCHW tensor: a view where the NHWC memory already has that order (one channel
    or one pixel), the HIP transpose otherwise"""
    if x.shape[1] == 1 or x.shape[2] * x.shape[3] == 1:
        return x.reshape(x.size(0), -1)
    return F_hip.flatten_nchw(x)


class StyleEncoder(nn.Module):
    """models/network_Style_GAN.py:12-43: Conv2d(5) without activation, ``log2(image_size) - 2`` stride-2 Conv2d(3) + InstanceNorm +
    ReLU that double the channels up to ``max_channels``, two more stride-2 Conv2d(3) + ReLU, then the two Linear heads on the
    flattened map.  Modules are created in the reference's order, so keys, their order and the seeded default init equal its."""

    def __init__(self, z_dim, image_size, max_channels=1024):
        super().__init__()
        in_dim, out_dim = IMAGE_CHANNEL, 64
        convs = [Conv2d(in_dim, out_dim, 5, 1, activate=None)]
        for _ in range(_n_level(image_size)):
            in_dim, out_dim = out_dim, min(out_dim * 2, max_channels)
            convs.append(Conv2d(in_dim, out_dim, 3, stride=2, bn="instance"))
        convs.append(Conv2d(out_dim, out_dim, 3, stride=2))
        convs.append(Conv2d(out_dim, out_dim, 3, stride=2))
        self.convs = nn.Sequential(*convs)
        self.fc_mu = Linear(out_dim, z_dim, activate=None)
        self.fc_logvar = Linear(out_dim, z_dim, activate=None)

    def forward(self, x):
        x = _flatten(self.convs(x))
        return self.fc_mu(x), self.fc_logvar(x)


class Discriminator(nn.Module):
    """models/network_Style_GAN.py:201-229: the image and the content image side by side through Conv2d(5) + ReLU and
    ``log2(image_size) - 2`` stride-2 Conv2d(3) + InstanceNorm + ReLU, then two heads of two stride-2 Conv2d(3) each: one number
    through a sigmoid, ``num_of_classes`` numbers through a softmax.  The first layer of each head stays a Conv2d block of its own;
    the second layers, which see 2 x 2 maps at every power-of-two ``image_size``, run with their sigmoid and softmax as one
    kernel (functional.twin_head).  Modules are created in the reference's order."""

    def __init__(self, image_size, num_of_classes, max_channels=256):
        super().__init__()
        in_dim, out_dim = IMAGE_CHANNEL * 2, 64
        convs = [Conv2d(in_dim, out_dim, 5, 1)]
        for _ in range(_n_level(image_size)):
            in_dim, out_dim = out_dim, min(out_dim * 2, max_channels)
            convs.append(Conv2d(in_dim, out_dim, 3, stride=2, bn="instance"))
        self.convs = nn.Sequential(*convs)
        self.adv_convs = nn.Sequential(Conv2d(out_dim, out_dim, 3, stride=2, activate="lrelu"),
                                       Conv2d(out_dim, 1, 3, stride=2, activate=None))
        self.aux_convs = nn.Sequential(Conv2d(out_dim, out_dim, 3, stride=2, activate="lrelu"),
                                       Conv2d(out_dim, num_of_classes, 3, stride=2, activate=None))
        self.num_of_classes, self.head_channels = num_of_classes, out_dim

    def _trunk_size(self, n):
        for _ in range(len(self.convs) - 1):
            n = (n - 1) // 2 + 1
        return n

    def uses_fused_head(self, x, x_content) -> bool:
        """Does forward(x, x_content, y) take functional.twin_head?  The switch on, a 4 x 4 trunk output (so that the last layer
        of each head sees 2 x 2), class and channel counts inside the kernel's range, fp32 tensors."""
        return bool(_HEAD_FUSED and x.dim() == 4 and self._trunk_size(x.shape[2]) == 4 and self._trunk_size(x.shape[3]) == 4
                    and 1 <= self.num_of_classes <= _HEAD_MAX_K and 1 <= self.head_channels <= _HEAD_MAX_C
                    and x.dtype == torch.float32 and x_content.dtype == torch.float32
                    and self.adv_convs[1].conv[0].weight.dtype == torch.float32)

    def forward(self, x, x_content, y):
        fused = self.uses_fused_head(x, x_content)
        x = self.convs(torch.cat([x, x_content], dim=1))
        if fused:
            pa, pu = self.adv_convs[1].conv[0], self.aux_convs[1].conv[0]
            return F_hip.twin_head(self.adv_convs[0](x), self.aux_convs[0](x), pa.weight, pa.bias, pu.weight, pu.bias)
        adv_res = F_hip.activation(_flatten(self.adv_convs(x)), "sigmoid")
        aux_res = F_hip.softmax_rows(_flatten(self.aux_convs(x)))
        return adv_res, aux_res
