"""What the fused font-inference tests share: seeded nets with non-trivial eval state, the fp64 oracle (oracle/ref_font.py, imported as
it is) evaluated once per case, and the cases of the whole-image convolution + InstanceNorm kernel."""
import functools

import torch
import torch.nn.functional as F

BATCH = 3
LRELU = 0.02          # blocks._CONV_LRELU
# the whole-image kernel's cases: (B, input H, W, Cin, Cout, ks, stride, act).  4x4 maps with 3 of 16 slots; two tiles with a partial
# second one; a stride-2 layer; a 1x1 layer on a one-image tile; the longest K of ComposeNet(64) (cat.3: 9 * 1024)
CONV_IN_CASES = [(3, 4, 4, 64, 64, 3, 1, "relu"), (17, 4, 4, 64, 128, 3, 1, "lrelu"), (5, 16, 16, 64, 64, 3, 2, "relu"),
                 (2, 16, 16, 128, 64, 1, 1, None), (3, 8, 8, 1024, 64, 3, 1, "relu")]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f64(p):
    return {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in p.items()}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def act64(y, act):
    if act == "relu":
        return torch.relu(y)
    if act == "lrelu":
        return F.leaky_relu(y, LRELU)
    return y


@functools.lru_cache(maxsize=None)
def conv_in_case(i):
    """(x NHWC fp32 with one all-zero image, w (Cout,Cin,k,k) fp32 with one all-zero output channel, fp64 reference NCHW)"""
    B, H, W, Cin, Cout, ks, stride, act = CONV_IN_CASES[i]
    g = gen(300 + i)
    x = torch.randn((B, Cin, H, W), generator=g)
    x[B // 2] = 0.0
    w = (torch.rand((Cout, Cin, ks, ks), generator=g) * 2 - 1) * (3.0 / (Cin * ks * ks)) ** 0.5
    w[Cout // 3] = 0.0
    with torch.no_grad():
        ref = act64(F.instance_norm(F.conv2d(x.double(), w.double(), None, stride=stride, padding=(ks - 1) // 2), eps=1e-5), act)
    return nhwc(x), w, ref


@functools.lru_cache(maxsize=None)
def seeded_net(S):
    """``networks_BE_font.ComposeNet(S)`` on the CPU in eval mode: ``seeded_weights(state_dict, 77)``, every running mean 0.1 randn and
    every running variance rand + 0.5 from one generator (seed 5) in key order -- default running statistics would hide a wrong fold"""
    from oracle import ref_font as RF
    from vae_play_amd import networks_BE_font as NF
    net = NF.ComposeNet(S)
    sd = RF.seeded_weights(net.state_dict(), 77)
    g = gen(5)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
    net.load_state_dict(sd)
    return net.eval()


@functools.lru_cache(maxsize=None)
def net_case(S):
    """(net, images (3,3,S,S), y, fp64 oracle results): {"none": logits with y=None, "y": logits with y, "cond_none": (label, style) of
    the style encoder, "cond_y": of the embedding block}.  Computed once; shared and not to be modified."""
    from oracle import ref_font as RF
    net = seeded_net(S)
    imgs, _, _, _, y = RF.synthetic_batch(BATCH, S)
    p = f64({k: v.detach() for k, v in net.state_dict().items()})
    x64, y64 = imgs.double(), {k: v.double() for k, v in y.items()}
    with torch.no_grad():
        ref = {"none": RF.compose_forward(p, x64, None, S, training=False), "y": RF.compose_forward(p, x64, y64, S, training=False),
               "cond_none": (RF.style_encode_block(p, "style_encoder.label_encode_block.", x64, S),
                             RF.style_encode_block(p, "style_encoder.style_encode_block.", x64, S)),
               "cond_y": (RF.embeding_block(p, "embeding_block.label_encode_block.", y64["cls"]),
                          RF.embeding_block(p, "embeding_block.style_encode_block.", y64["cnt_style"]))}
    return net, imgs, y, ref


def in_layers(net, S):
    """every convolution + InstanceNorm block of the net as (tag, Cin, Cout, ks, stride, input H = W), and every convolution +
    BatchNorm block as tags: walked from the modules, in the style-encoder (y=None) forward's order"""
    ins, bns = [], []

    def add(tag, block, H):
        conv = block.conv[0]
        ins.append((tag, conv.weight.shape[1], conv.weight.shape[0], conv.kernel_size, conv.stride, H))
        return (H + 2 * ((conv.kernel_size - 1) // 2) - conv.kernel_size) // conv.stride + 1

    for name in ("label_encode_block", "style_encode_block"):
        H = S
        for i, layer in enumerate(list(getattr(net.style_encoder, name).convs)[:-1]):
            H = add(f"style_encoder.{name}.convs.{i}", layer, H)
    H = add("down.0", net.down[0], S)
    sizes = [H]
    for k in range(1, len(net.down)):
        bns.append(f"down.{k}.0")
        H = add(f"down.{k}.1", net.down[k][1], H // 2)
        sizes.append(H)
    for k in reversed(range(len(net.up))):
        bns += [f"up.{k}.conv.0", f"up.{k}.conv.1"]
        add(f"skip.{k}", net.skip[k], sizes[k])
        add(f"cat.{k}", net.cat[k], sizes[k])
    for head in ("edge_net", "mask_net"):
        for i in (0, 1):
            add(f"{head}.predictor.{i}", getattr(net, head).predictor[i], S)
    return ins, bns
