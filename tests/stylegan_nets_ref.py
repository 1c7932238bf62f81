"""fp64 restatement of the Style-GAN StyleEncoder and Discriminator forwards (models/network_Style_GAN.py:12-43 and :201-229 of the
reference) in plain torch.nn.functional on the CPU: they take a ``state_dict``; autograd supplies the gradients.  Written from the
reference's arithmetic, independent of the package under test (no HIP, no vae_play_amd import)."""
import torch
import torch.nn.functional as F

from tests.util import load_golden


def conv_block(sd, pre, x, stride=1, bn=None, act="relu"):
    """blocks.Conv2d: convolution with padding (k - 1) // 2, bias iff bn is None, InstanceNorm2d(eps 1e-5), ReLU | LeakyReLU(0.02)"""
    w = sd[pre + ".conv.0.weight"]
    y = F.conv2d(x, w, sd.get(pre + ".conv.0.bias"), stride=stride, padding=(w.shape[2] - 1) // 2)
    if bn == "instance":
        y = F.instance_norm(y, eps=1e-5)
    if act == "relu":
        return F.relu(y)
    return F.leaky_relu(y, 0.02) if act == "lrelu" else y


def _levels(sd, pre):
    """indices of the stride-2 InstanceNorm convolutions of ``pre``: the blocks after the first that have no bias"""
    n = 1
    while f"{pre}.{n}.conv.0.weight" in sd and f"{pre}.{n}.conv.0.bias" not in sd:
        n += 1
    return range(1, n)


def encoder_forward(sd, x):
    h = conv_block(sd, "convs.0", x, act=None)
    lv = _levels(sd, "convs")
    for i in lv:
        h = conv_block(sd, f"convs.{i}", h, 2, "instance")
    for i in (lv.stop, lv.stop + 1):
        h = conv_block(sd, f"convs.{i}", h, 2)
    h = h.reshape(h.shape[0], -1)
    return (F.linear(h, sd["fc_mu.fc.0.weight"], sd["fc_mu.fc.0.bias"]),
            F.linear(h, sd["fc_logvar.fc.0.weight"], sd["fc_logvar.fc.0.bias"]))


def discriminator_forward(sd, x, x_content):
    B = x.shape[0]
    h = conv_block(sd, "convs.0", torch.cat([x, x_content], dim=1))
    for i in _levels(sd, "convs"):
        h = conv_block(sd, f"convs.{i}", h, 2, "instance")
    a = conv_block(sd, "adv_convs.1", conv_block(sd, "adv_convs.0", h, 2, act="lrelu"), 2, act=None)
    u = conv_block(sd, "aux_convs.1", conv_block(sd, "aux_convs.0", h, 2, act="lrelu"), 2, act=None)
    return torch.sigmoid(a.reshape(B, -1)), torch.softmax(u.reshape(B, -1), dim=-1)


def run(forward, state_dict, inputs, grads):
    """fp64 forward + backward of sum_i sum(out_i * grads[i]) with ``state_dict``'s values: (outputs, input gradients,
    {key: parameter gradient})"""
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in state_dict.items()}
    leaves = [v.detach().cpu().double().requires_grad_(True) for v in inputs]
    outs = forward(sd, *leaves)
    torch.autograd.backward(list(outs), [g.detach().cpu().double() for g in grads])
    return [o.detach() for o in outs], [l.grad for l in leaves], {k: v.grad for k, v in sd.items()}


FIXTURES = {"encoder": ("stylegan_encoder_16_z8", encoder_forward, ("x",), ("g_mu", "g_logvar"), ("mu", "logvar"), ("dx",)),
            "disc": ("stylegan_disc_16_k3", discriminator_forward, ("x", "x_content"), ("g_adv", "g_aux"), ("adv", "aux"),
                     ("dx", "dx_content"))}
_CACHE = {}


def fixture(which):
    """the fixture's arrays, with ``params``: its state_dict in key order"""
    if ("g", which) not in _CACHE:
        g = load_golden(FIXTURES[which][0])
        g["params"] = {str(k): torch.from_numpy(g[f"param/{k}"]) for k in g["keys"]}
        _CACHE["g", which] = g
    return _CACHE["g", which]


def reference(which):
    """``run`` on the fixture's own parameters, inputs and output gradients; computed once per process and shared, unchanged, by
    the tests that need it"""
    if ("ref", which) not in _CACHE:
        g = fixture(which)
        _, fwd, n_in, n_g, _, _ = FIXTURES[which]
        _CACHE["ref", which] = run(fwd, g["params"], [torch.from_numpy(g[k]) for k in n_in], [torch.from_numpy(g[k]) for k in n_g])
    return _CACHE["ref", which]
