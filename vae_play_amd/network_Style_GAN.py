"""Drop-in classes for kungyao/vae-play's ``models/network_Style_GAN.py`` on the HIP back end: the 4x4 stride-2 transposed
convolution of the Style-GAN generator and its first user, the decoder block.

Same constructor signatures and ``state_dict`` keys as the reference:
  ConvTranspose2d(in, out, 4, 2, 1)  nn.ConvTranspose2d with its default bias                    models/network_Style_GAN.py:49,116
     keys weight (in, out, 4, 4), bias (out); the bias is added in the scatter kernel's epilogue
  StyleUp(in_channel, out_channel)                                                               models/network_Style_GAN.py:45-65
     keys up_convs.0.{weight,bias}, cat_convs.0.conv.0.{weight,bias}, cat_convs.{1,2}.{cSE.1,cSE.3,sSE.0}.{weight,bias}
The rest of the reference module (StyleEncoder, myConv2d, Generator, MLP, Discriminator) has no drop-in here yet;
``blocks.Conv2d(in, out, 4, 2, bn="instance")`` is the convolution inside myConv2d (:95-98).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import functional as F_hip
from .blocks import Conv2d, SCSEBlock, _NoParams


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
