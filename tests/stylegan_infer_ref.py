"""What the fused Style-GAN inference tests share: seeded nets, inputs and the fp64 results of the existing restatements
(tests/stylegan_ref.generator_forward, tests/stylegan_nets_ref.encoder_forward / discriminator_forward, imported as they are), each
evaluated once per size; the cases of the twin-SCSE kernel with its fp64 two-pass form.  Nothing here touches the HIP library."""
import functools

import torch
import torch.nn.functional as F

from tests.stylegan_nets_ref import discriminator_forward, encoder_forward
from tests.stylegan_ref import generator_forward, scse

BATCH, Z, CLASSES = 3, 8, 2
SIZES = (32, 64)
LABELS = (0.0, 1.0, 0.25)
# vp_scse2_fwd_f32: (B, C, H, W, reduction).  A small float4 case; the scalar path; several chunks per image; the largest C; the
# scalar path near its C limit; a tiny C
SCSE2_CASES = [(2, 32, 5, 7, 4), (3, 70, 9, 11, 5), (2, 64, 64, 64, 4), (1, 1024, 3, 5, 16), (2, 250, 6, 5, 5), (2, 6, 17, 13, 2)]
SCSE_KEYS = ("cSE.1.weight", "cSE.1.bias", "cSE.3.weight", "cSE.3.bias", "sSE.0.weight", "sSE.0.bias")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f64(sd):
    return {k: v.detach().double() for k, v in sd.items()}


# ---- the two SCSE blocks -------------------------------------------------------------------------------------------------------------
def scse_params(C, hidden, g, pre):
    """one block's six parameters as nn.Conv2d stores them, under ``pre``: signed, of the size default init gives"""
    def u(*shape, fan):
        return (torch.rand(shape, generator=g) * 2 - 1) / fan ** 0.5
    return {f"{pre}.cSE.1.weight": u(hidden, C, 1, 1, fan=C), f"{pre}.cSE.1.bias": u(hidden, fan=C),
            f"{pre}.cSE.3.weight": u(C, hidden, 1, 1, fan=hidden), f"{pre}.cSE.3.bias": u(C, fan=hidden),
            f"{pre}.sSE.0.weight": u(1, C, 1, 1, fan=C), f"{pre}.sSE.0.bias": u(1, fan=C)}


def scse2_direct(sd, x, relu):
    """relu?(scse_b(scse_a(x))) by the existing restatement of one block, NCHW"""
    y = scse(sd, "b", scse(sd, "a", x))
    return F.relu(y) if relu else y


def scse2_two_pass(sd, x, relu):
    """the same in the form the kernel computes: ONE read of x gives sum x and sum x s_a, hence block b's pooled input
    c_a mean(x) + mean(x s_a); a second read forms y_a, s_b from y_a, and y"""
    def gate(pre, pool):
        h = F.relu(F.conv2d(pool, sd[f"{pre}.cSE.1.weight"], sd[f"{pre}.cSE.1.bias"]))
        return torch.sigmoid(F.conv2d(h, sd[f"{pre}.cSE.3.weight"], sd[f"{pre}.cSE.3.bias"]))
    # pass 1
    s_a = torch.sigmoid(F.conv2d(x, sd["a.sSE.0.weight"], sd["a.sSE.0.bias"]))
    mean_x, mean_xs = x.mean((2, 3), keepdim=True), (x * s_a).mean((2, 3), keepdim=True)
    # gates
    c_a = gate("a", mean_x)
    c_b = gate("b", c_a * mean_x + mean_xs)
    # pass 2
    y_a = x * (c_a + torch.sigmoid(F.conv2d(x, sd["a.sSE.0.weight"], sd["a.sSE.0.bias"])))
    y = y_a * (c_b + torch.sigmoid(F.conv2d(y_a, sd["b.sSE.0.weight"], sd["b.sSE.0.bias"])))
    return F.relu(y) if relu else y


@functools.lru_cache(maxsize=None)
def scse2_case(i):
    """(x NCHW fp32 signed, with image 0 all zero when B > 1; the two blocks' parameters fp32; fp64 results without and with ReLU)"""
    B, C, H, W, red = SCSE2_CASES[i]
    g = gen(1700 + i)
    x = torch.randn((B, C, H, W), generator=g)
    if B > 1:
        x[0] = 0.0
    sd = {**scse_params(C, C // red, g, "a"), **scse_params(C, C // red, g, "b")}
    with torch.no_grad():
        ref = {r: scse2_direct(f64(sd), x.double(), r) for r in (0, 1)}
    return x, sd, ref


# ---- the nets ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seeded_nets(S):
    """(Generator(S, 8), StyleEncoder(8, S), Discriminator(S, 2)) on the CPU with their seeded default init"""
    from vae_play_amd import network_Style_GAN as N
    torch.manual_seed(4100 + S)
    return N.Generator(S, Z), N.StyleEncoder(Z, S), N.Discriminator(S, CLASSES)


@functools.lru_cache(maxsize=None)
def net_case(S):
    """(nets, inputs, fp64 results).  inputs: x_content, x_style, x (3, 3, S, S), z, eps (3, 8), labels (3,).  results: generate with
    the mixed labels and with all 0 / all 1 ("generate", "generate0", "generate1"), mu, logvar, stylize with eps, adv, aux.  Computed
    once; shared and not to be modified."""
    G, E, D = seeded_nets(S)
    g = gen(4200 + S)
    inp = {"x_content": torch.rand((BATCH, 3, S, S), generator=g), "x_style": torch.rand((BATCH, 3, S, S), generator=g),
           "x": torch.rand((BATCH, 3, S, S), generator=g) * 2 - 1, "z": torch.randn((BATCH, Z), generator=g),
           "eps": torch.randn((BATCH, Z), generator=g), "labels": torch.tensor(LABELS)}
    sg, se, sd_ = f64(G.state_dict()), f64(E.state_dict()), f64(D.state_dict())
    d = {k: v.double() for k, v in inp.items()}
    with torch.no_grad():
        ref = {"generate": generator_forward(sg, d["x_content"], d["z"], d["labels"], S)}
        for c in (0, 1):
            ref[f"generate{c}"] = generator_forward(sg, d["x_content"], d["z"], torch.full((BATCH,), float(c), dtype=torch.float64), S)
        ref["mu"], ref["logvar"] = encoder_forward(se, d["x_style"])
        z = ref["mu"] + d["eps"] * torch.exp(ref["logvar"] / 2)
        ref["stylize"] = generator_forward(sg, d["x_content"], z, d["labels"], S)
        ref["adv"], ref["aux"] = discriminator_forward(sd_, d["x"], d["x_content"])
    return (G, E, D), inp, ref
