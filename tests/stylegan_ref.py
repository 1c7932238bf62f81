"""fp64 restatement of the Style-GAN generator's forward (models/network_Style_GAN.py:45-199 of the reference) in plain
torch.nn.functional on the CPU: it takes a ``state_dict``; autograd supplies the gradients.  Written from the reference's
arithmetic, independent of the package under test (no HIP, no vae_play_amd import)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.util import GOLDEN

ZERO_BIAS = tuple(f"up{i}.up_convs.0.bias" for i in (1, 2, 3))    # InstanceNorm follows: their gradient is mathematically zero


def load_generator_fixture():
    """stylegan_generator_32_z8.npz merged with its shard files (param/<key>, grad/<key> of the small tensors)"""
    g = dict(np.load(f"{GOLDEN}/stylegan_generator_32_z8.npz"))
    i = 0
    while True:
        try:
            g.update(np.load(f"{GOLDEN}/stylegan_generator_32_z8_p{i}.npz"))
        except FileNotFoundError:
            return g
        i += 1


def conv_block(sd, pre, x, stride=1, bn=None, act="relu"):
    """blocks.Conv2d: convolution with padding (k - 1) // 2, bias iff bn is None, InstanceNorm2d(eps 1e-5), activation"""
    w = sd[pre + ".conv.0.weight"]
    y = F.conv2d(x, w, sd.get(pre + ".conv.0.bias"), stride=stride, padding=(w.shape[2] - 1) // 2)
    if bn == "instance":
        y = F.instance_norm(y, eps=1e-5)
    return F.relu(y) if act == "relu" else y


def my_conv(sd, pre, x, label, stride=1, bn=None, act="relu"):
    return (conv_block(sd, pre + ".conv_1", x, stride, bn, act) * (1 - label)
            + conv_block(sd, pre + ".conv_2", x, stride, bn, act) * label)


def scse(sd, pre, x):
    c = x.mean((2, 3), keepdim=True)
    c = F.relu(F.conv2d(c, sd[pre + ".cSE.1.weight"], sd[pre + ".cSE.1.bias"]))
    c = torch.sigmoid(F.conv2d(c, sd[pre + ".cSE.3.weight"], sd[pre + ".cSE.3.bias"]))
    s = torch.sigmoid(F.conv2d(x, sd[pre + ".sSE.0.weight"], sd[pre + ".sSE.0.bias"]))
    return x * c + x * s


def style_up(sd, pre, x, skip):
    x = F.conv_transpose2d(x, sd[pre + ".up_convs.0.weight"], sd[pre + ".up_convs.0.bias"], stride=2, padding=1)
    x = F.relu(F.instance_norm(x, eps=1e-5))
    x = conv_block(sd, pre + ".cat_convs.0", torch.cat([x, skip], dim=1))
    return F.relu(scse(sd, pre + ".cat_convs.2", scse(sd, pre + ".cat_convs.1", x)))


def generator_forward(sd, x, style, labels, image_size):
    B = x.shape[0]
    s = style.reshape(B, -1)
    for i in range(3):
        s = F.linear(s, sd[f"mlp.model.{i}.fc.0.weight"], sd[f"mlp.model.{i}.fc.0.bias"])
    h = torch.cat([x, s.reshape(B, 1, image_size, image_size)], dim=1)
    lab = labels.reshape(B, 1, 1, 1).to(x.dtype)
    c0 = my_conv(sd, "conv2", my_conv(sd, "conv1", h, lab, act=None), lab, act=None)
    d1 = my_conv(sd, "down1", c0, lab, 2, "instance")
    d2 = my_conv(sd, "down2", d1, lab, 2, "instance")
    d3 = my_conv(sd, "down3", d2, lab, 2, "instance")
    d4 = my_conv(sd, "down4", d3, lab, 2, "instance")
    u1 = style_up(sd, "up1", d4, conv_block(sd, "skip1", d3, bn="instance"))
    u2 = style_up(sd, "up2", u1, conv_block(sd, "skip2", d2, bn="instance"))
    u3 = style_up(sd, "up3", u2, conv_block(sd, "skip3", d1, bn="instance"))
    y = F.conv_transpose2d(u3, sd["final.0.weight"], sd["final.0.bias"], stride=2, padding=1)
    y = conv_block(sd, "final.2", conv_block(sd, "final.1", y))
    return torch.tanh(conv_block(sd, "final.3", y, act=None))


_CACHE = {}


def generator_reference(state_dict, g):
    """fp64 forward + backward of the fixture's inputs with ``state_dict``'s values: {"y", "dx", "dstyle", "grad/<key>"}; computed
    once per process (the fixture's seed fixes the parameters) and shared, unchanged, by the tests that need it"""
    if "ref" not in _CACHE:
        sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in state_dict.items()}
        x = torch.from_numpy(g["x"]).double().requires_grad_(True)
        style = torch.from_numpy(g["style"]).double().requires_grad_(True)
        y = generator_forward(sd, x, style, torch.from_numpy(g["labels"]), 32)
        y.backward(torch.from_numpy(g["gy"]).double())
        out = {"y": y.detach(), "dx": x.grad, "dstyle": style.grad}
        out.update({f"grad/{k}": v.grad for k, v in sd.items()})
        _CACHE["ref"] = out
    return _CACHE["ref"]
