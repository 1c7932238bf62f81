"""CPU emulation of the one-product fp16 inference arithmetic (FusedVAEInference(precision="f16")), torch only.

The eval-mode forward of the CPU oracle (oracle/ref_cpu.py) in fp64, in which every layer the "f16" plan runs on fp16 planes -- the
stride-2 blocks of the encoder (the im2col stem included) and of the decoder -- first rounds its input activation and its weight to
fp16: round to nearest even on 11 significant bits, saturating at +-65504, subnormal step 2^-24 below 2^-14 (csrc/split.h split_f16's
hi plane).  Products of two such values are exact in fp32, and the kernels accumulate in fp32; the emulation accumulates in fp64, so
what it measures is the error of the operand rounding alone -- the part of the mode's error that no kernel can remove.  The final
convolution, the dense layers and every BatchNorm keep full precision, as in the plan.
"""
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O

F16_MAX = 65504.0


def round_f16(t: torch.Tensor) -> torch.Tensor:
    """t (fp64) -> the fp16 hi plane's value, as fp64"""
    return t.clamp(-F16_MAX, F16_MAX).to(torch.float16).double()


def _block(p, prefix, x, transposed, rounded):
    w = p[prefix + ".conv.weight"]
    if rounded:
        x, w = round_f16(x), round_f16(w)
    if transposed:
        y = F.conv_transpose2d(x, w, None, stride=2, padding=2, output_padding=1)
    else:
        y = F.conv2d(x, w, None, stride=2, padding=2)
    return F.relu(O._bn(p, prefix + ".bn", y, False))


def encoder_forward(p, x, L, rounded=True, prefix="encoder."):
    t = x
    for i in range(L):
        t = _block(p, f"{prefix}conv.{i}", t, False, rounded)
    t = t.reshape(len(t), -1)
    t = F.linear(t, p[prefix + "fc.0.weight"])
    t = F.relu(O._bn(p, prefix + "fc.1", t, False))
    return F.linear(t, p[prefix + "l_mu.weight"], p[prefix + "l_mu.bias"]), F.linear(t, p[prefix + "l_var.weight"], p[prefix + "l_var.bias"])


def decoder_forward(p, z, L, rounded=True, prefix="decoder."):
    t = F.linear(z, p[prefix + "fc.0.weight"])
    t = F.relu(O._bn(p, prefix + "fc.1", t, False))
    t = t.view(len(t), -1, 8, 8)
    for i in range(L):
        t = _block(p, f"{prefix}conv.{i}", t, True, rounded)
    t = F.conv2d(t, p[f"{prefix}conv.{L}.0.weight"], p[f"{prefix}conv.{L}.0.bias"], stride=1, padding=2)
    return torch.sigmoid(t)


def vae_forward(p, x, eps, L, rounded=True):
    """{mu, logvar, z, x_tilde} of the eval-mode forward; ``p`` holds fp64 tensors.  ``rounded=False`` is the oracle itself."""
    with torch.no_grad():
        mu, logvar = encoder_forward(p, x, L, rounded)
        z = O.reparameterize(mu, logvar, eps)
        return {"mu": mu, "logvar": logvar, "z": z, "x_tilde": decoder_forward(p, z, L, rounded)}
