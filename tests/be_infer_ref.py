"""What the fused segmentation-inference tests share: the shape set, seeded blocks and nets with non-trivial eval state, and the fp64
oracle (oracle/ref_be.py, oracle/ref_cpu.py, imported as they are) evaluated once per case."""
import functools

import torch

TH, TW = 8, 16        # the head kernels' tile (csrc/be_infer.h; tests/test_be_infer_cpu.py checks these against the compiled header)
# feature-map shapes (feat_h, feat_w), batch 2: one pixel; smaller than a tile with odd sizes; one exact tile; one row and one column
# past a tile edge; four tiles in each direction with a one-pixel last tile (tiles with all eight neighbours exist)
SHAPES = [(1, 1), (3, 5), (TH, TW), (TH + 1, TW + 1), (3 * TH + 1, 3 * TW + 1)]
BATCH = 2
WIDTHS = (16, 32, 64)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _bn(p, prefix, c, g):
    """gamma ~ U(0.5, 1.5), beta ~ N(0, 0.2), running mean ~ N(0, 0.5), running variance ~ U(0.5, 2): with the default 0 / 1 buffers
    "outside the image is 0, not relu(shift)" could not fail"""
    p[prefix + "weight"] = torch.empty(c).uniform_(0.5, 1.5, generator=g)
    p[prefix + "bias"] = torch.randn(c, generator=g) * 0.2
    p[prefix + "running_mean"] = torch.randn(c, generator=g) * 0.5
    p[prefix + "running_var"] = torch.empty(c).uniform_(0.5, 2.0, generator=g)


def _conv_w(cout, cin, g):
    bound = (6.0 / (cin * 9)) ** 0.5
    return (torch.rand((cout, cin, 3, 3), generator=g) * 2 - 1) * bound


def up_params(cin, cmid, seed, prefix="", coord_gain=0.05):
    """fp32 parameters of one Up(cin, cmid, if_add_coord=True) keyed like the reference's state_dict.  The weights of the two
    coordinate channels are scaled down: their inputs reach the map's width, the others are O(1), and the test should see both."""
    g, p = gen(seed), {}
    w1 = _conv_w(cmid, cin + 2, g)
    w1[:, cin:] *= coord_gain
    p[prefix + "conv.0.conv.0.weight"] = w1
    _bn(p, prefix + "conv.0.conv.1.", cmid, g)
    p[prefix + "conv.1.conv.0.weight"] = _conv_w(cmid, cmid, g)
    _bn(p, prefix + "conv.1.conv.1.", cmid, g)
    return p


def pred_params(c, seed, prefix=""):
    g, p = gen(seed), {}
    for i, (ci, co) in enumerate(((c, 2 * c), (2 * c, c), (c, 1))):
        p[f"{prefix}predictor.{i}.conv.0.weight"] = _conv_w(co, ci, g)
        p[f"{prefix}predictor.{i}.conv.0.bias"] = torch.randn(co, generator=g) * 0.3       # (the reference initialises them to 0)
    return p


def head_params(width, seed, prefix=""):
    p = up_params(width, width // 4, seed, prefix + "conv1.")
    p.update(up_params(width // 4, width // 8, seed + 1, prefix + "conv2."))
    p.update(pred_params(width // 8, seed + 2, prefix))
    return p


def f64(p):
    return {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in p.items()}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def head_case(width, h, w):
    """One case of the kernel tests: two heads' parameters, a feature map, and the fp64 oracle's output of every stage per head
    (models/networks_BE.py:54-58 in eval mode).  Each stage's fp32 input is the oracle's previous output rounded to fp32, so the three
    kernels are held to the single-op bar one by one.  Computed once; the tensors are shared and must not be modified."""
    from oracle import ref_cpu as O
    heads = [head_params(width, 10 * width + 3 * k) for k in range(2)]
    x = torch.randn((BATCH, width, h, w), generator=gen(1000 + width + 7 * h + w))
    case = {"params": heads, "x": x, "u1_in": [], "u1": [], "u2": [], "logits": []}
    with torch.no_grad():
        for p in heads:
            p64 = f64(p)
            u1 = O.blocks_up(p64, "conv1.", x.double(), True, False)
            u1_in = u1.float()
            u2 = O.blocks_up(p64, "conv2.", u1_in.double(), True, False)
            y = u2.float().double()
            for i in range(3):
                y = O.blocks_conv2d(p64, f"predictor.{i}.", y, 3, 1, None, None, False)
            case["u1"].append(u1)
            case["u1_in"].append(u1_in)
            case["u2"].append(u2)
            case["logits"].append(y)
    return case


# ---- whole nets ----------------------------------------------------------------------------------------------------------------------
def seeded_net(kind, feat_channels=256, seed=0):
    """``networks_BE.ComposeNet`` (kind "be": 256-channel feature, head width 32) or ``networks_BE_GAN.ComposeNet`` ("gan": width 64)
    on the CPU, no backbone, with non-trivial eval state from a fixed seed: every BatchNorm's running statistics and affine parameters
    and every predictor bias random (tests/be_infer_ref._bn); the coordinate channels' weights scaled as in ``up_params``"""
    from vae_play_amd import networks_BE, networks_BE_GAN
    torch.manual_seed(seed)
    if kind == "be":
        net = networks_BE.ComposeNet(networks_BE.FeatureNet(None, feat_channels, 32))
    else:
        net = networks_BE_GAN.ComposeNet(3, 128, None, feat_channels)
    g = gen(500 + seed)
    with torch.no_grad():
        for name, m in net.named_modules():
            if hasattr(m, "num_batches_tracked"):
                p = {}
                _bn(p, "", m.weight.numel(), g)
                for k, v in p.items():
                    getattr(m, k).copy_(v)
        for name, q in net.named_parameters():
            if ".predictor." in name and name.endswith(".bias"):
                q.copy_(torch.randn(q.shape, generator=g) * 0.3)
            if name.endswith("conv.0.conv.0.weight") and (".conv1." in name or ".conv2." in name):
                q[:, -2:] *= 0.05
    return net.eval()


def net_state64(net):
    """the net's state as the oracle's fp64 parameter dict, ``aux_convs.`` / ``mask_net.`` / ``edge_net.`` keys"""
    return {k.replace("feature_net.", ""): (v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu().clone())
            for k, v in net.state_dict().items()}


def oracle_net(net, x, feat_channels=256):
    """fp64 eval-mode {"features", "edges", "masks"} of the CPU oracle on the net's state"""
    from oracle import ref_be as RB
    p = net_state64(net)
    width = p["mask_net.conv1.conv.0.conv.0.weight"].shape[1] - 2
    with torch.no_grad():
        f = RB.aux_convs_forward(p, x.detach().cpu().double(), feat_channels, width, False, "aux_convs.")
        return {"features": f, "edges": RB.masknet_forward(p, f, False, "edge_net."), "masks": RB.masknet_forward(p, f, False, "mask_net.")}
