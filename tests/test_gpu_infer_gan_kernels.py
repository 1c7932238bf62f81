"""The kernels of fused VAE-GAN inference called directly (csrc/infer_gan.hip and the planes-writing stem of csrc/edge.hip), every
output between guard elements (tests/guarded.py): a store outside the buffer shows as a clobbered guard, an element never written as
a NaN that is left."""
import itertools

import pytest
import torch

from tests import conv_ref, small_ref
from tests.guarded import Guards, gen, same_bits, scalar_close, tensor_close
from tests.util import record, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- K1: the stem writing split planes ---------------------------------------------------------------------------------------------
# a partial row tile and a partial column tile (tiles are 8 x 32 pixels), a width under one tile, both channel counts, both input counts
K1_SHAPES = [(2, 9, 40, 1, 32), (1, 16, 16, 1, 32), (3, 8, 32, 3, 64), (1, 17, 33, 1, 64)]


@pytest.mark.parametrize("B,H,W,Cs,Cb", K1_SHAPES)
@pytest.mark.parametrize("act,with_bias", [(1, True), (0, True), (1, False), (0, False)])
def test_stem_planes_equal_the_split_of_the_fp32_entry_point(B, H, W, Cs, Cb, act, with_bias):
    from vae_play_amd import ops
    g = gen(31 + H + Cb + Cs)
    x = torch.rand(B, Cs, H, W, generator=g)
    w = (torch.rand(Cb, Cs, 5, 5, generator=g) - 0.5) * 0.4
    bias = (torch.rand(Cb, generator=g) - 0.5) if with_bias else None
    xd, wd = ops.channels_last(x.to(DEV)), w.to(DEV)
    bd = bias.to(DEV) if with_bias else None
    n = B * H * W * Cb
    G = Guards()
    planes = G.planes("planes", n)
    ops.conv5_smallin_fwd_planes_bf16x3(xd, wd, bd, act, out=planes)
    G.check()
    y = ops.conv5_smallin_fwd_bf16x3(xd, wd, bd, act)
    want = ops.split_f32(y)
    assert torch.equal(planes, want), f"{int((planes != want).sum())} of {2 * n} plane elements differ from vp_split_f32 of the fp32 result"
    # hi + lo against the fp64 direct sum, held to the bound tests/test_gpu_edge.py applies to the fp32 entry point
    pts = [(b, h, v) for b in range(B) for h in range(H) for v in range(W)]
    r, _ = conv_ref.gather_ref(x, w, pts, stride=1)
    if with_bias:
        r = r + bias.double()[None, :]
    if act == 1:
        r = r.clamp(min=0.0)
    got = conv_ref.take(ops.unsplit(planes).view(B, H, W, Cb).permute(0, 3, 1, 2).cpu(), pts)
    e = rel_err(got, r)
    record(f"stem planes {B}x{H}x{W} {Cs}->{Cb} act{act}", e)
    print(f"stem planes {B}x{H}x{W} {Cs}->{Cb} act{act} bias{int(with_bias)}: {e:.3e}")
    assert e <= 3e-5


def test_stem_planes_two_halves_fill_one_split_tensor():
    """the way the plan calls it: one launch per half, each with its own source, into consecutive pieces of one split tensor"""
    from vae_play_amd import _lib, ops
    B, S, C0 = 2, 16, 32
    g = gen(5)
    xa, xb = torch.rand(B, 1, S, S, generator=g).to(DEV), torch.rand(B, 1, S, S, generator=g).to(DEV)
    w, bias = ((torch.rand(C0, 1, 5, 5, generator=g) - 0.5) * 0.4).to(DEV), (torch.rand(C0, generator=g) - 0.5).to(DEV)
    half = B * S * S * C0
    G = Guards()
    planes = G.planes("planes", 2 * half)
    for k, src in enumerate((xa, xb)):
        _lib.call("vp_conv5_smallin_fwd_planes_bf16x3", ops._p(src), ops._p(w), ops._p(bias), ops.c_void_p(planes.data_ptr() + 2 * k * half),
                  2 * half, B, S, S, 1, C0, 1, ops._stream())
    G.check()
    y = ops.conv5_smallin_fwd_bf16x3(ops.channels_last(torch.cat([xa, xb])), w, bias, 1)
    assert torch.equal(planes, ops.split_f32(y))
    with pytest.raises(_lib.VaePlayHipError, match="overlap"):
        _lib.call("vp_conv5_smallin_fwd_planes_bf16x3", ops._p(xa), ops._p(w), ops._p(bias), ops._pv(planes), half - 1, B, S, S, 1, C0, 1,
                  ops._stream())


# ---- K2: the tap ---------------------------------------------------------------------------------------------------------------------
def _tap_inputs(n, C, seed=0):
    g = gen(100 + n + C + seed)
    c = torch.randn(n, 64, C, generator=g)
    scale = torch.rand(C, generator=g) + 0.5
    scale[::3] *= -1.0                      # negative ...
    scale[1::7] = 0.0                       # ... and zero scales
    shift = torch.randn(C, generator=g) * 0.3
    return c.to(DEV), scale.to(DEV), shift.to(DEV)


def _tap_three_launches(c, scale, shift):
    """the path the tap kernel replaces: vp_bn_act_fwd_f32 in eval form -- with mean 0 and rstd 1 its fma(gamma, (x - 0) * 1, beta) IS
    fma(c, s, t) -- then vp_nhwc_to_nchw_f32 of the activation, and of c for the features"""
    from vae_play_amd import _lib, ops
    n, _, C = c.shape
    P, st = ops._p, ops._stream()
    a = torch.empty_like(c)
    zeros, ones = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    _lib.call("vp_bn_act_fwd_f32", P(c), P(zeros), P(ones), P(scale), P(shift), P(a), n * 64, C, ops.ACT_RELU, 0.0, st)
    act, feat = torch.empty(n, C * 64, device=DEV), torch.empty(n, C * 64, device=DEV)
    _lib.call("vp_nhwc_to_nchw_f32", P(a), P(act), n, C, 8, 8, st)
    _lib.call("vp_nhwc_to_nchw_f32", P(c), P(feat), n, C, 8, 8, st)
    return act, feat


def _run_tap(c, scale, shift, want_act, want_feat, P):
    from vae_play_amd import ops
    n, _, C = c.shape
    G = Guards()
    act = G.out("act_flat", n, C * 64) if want_act else None
    feat = G.out("feat_flat", n, C * 64) if want_feat else None
    dist = G.out("dist", P) if P else None
    ops.disc_tap_eval(c, scale, shift, act, feat, P, dist)
    G.check()
    return act, feat, dist


@pytest.mark.parametrize("n,C", [(1, 32), (2, 64), (5, 128), (6, 256)])
def test_tap_equals_the_three_launches_it_replaces(n, C):
    c, scale, shift = _tap_inputs(n, C)
    act_ref, feat_ref = _tap_three_launches(c, scale, shift)
    cd = c.double().cpu()
    for P in sorted({0, n // 2 if n % 2 == 0 else 0}):
        for want_act, want_feat in itertools.product((True, False), repeat=2):
            if not (want_act or want_feat or P):
                continue
            act, feat, dist = _run_tap(c, scale, shift, want_act, want_feat, P)
            what = f"tap n{n} C{C} P{P} act{int(want_act)} feat{int(want_feat)}"
            if want_act:
                assert same_bits(act, act_ref), f"{what}: act_flat differs from vp_bn_act_fwd_f32 + vp_nhwc_to_nchw_f32"
            if want_feat:
                assert same_bits(feat, feat_ref), f"{what}: feat_flat differs from vp_nhwc_to_nchw_f32"
            if P:
                want = 0.5 * ((cd[:P] - cd[P:2 * P]) ** 2).sum((1, 2))
                scalar_close(dist, want, f"{what} dist")
                _, _, again = _run_tap(c, scale, shift, want_act, want_feat, P)
                assert same_bits(dist, again), f"{what}: two runs differ"


def test_tap_distance_does_not_depend_on_the_batch():
    """row i of an n = 6 call equals the n = 2 call on rows (i, i + P), bit for bit: the order of a pair's sum is its own"""
    c, scale, shift = _tap_inputs(6, 256)
    _, _, d6 = _run_tap(c, scale, shift, True, False, 3)
    for i in range(3):
        pair = torch.stack([c[i], c[i + 3]]).contiguous()
        a2, _, d2 = _run_tap(pair, scale, shift, True, False, 1)
        assert same_bits(d2, d6[i:i + 1]), f"pair {i}: {d2.item()!r} alone, {d6[i].item()!r} in the batch of 6"
    # rows beyond the pairs (n = 5, P = 2: row 4) are transposed like every other row
    c5, s5, t5 = _tap_inputs(5, 128)
    act_ref, feat_ref = _tap_three_launches(c5, s5, t5)
    act, feat, _ = _run_tap(c5, s5, t5, True, True, 2)
    assert same_bits(act, act_ref) and same_bits(feat, feat_ref)


def test_tap_argument_errors():
    from vae_play_amd import _lib, ops
    c, scale, shift = _tap_inputs(2, 32)
    out = torch.empty(2, 32 * 64, device=DEV)
    with pytest.raises(_lib.VaePlayHipError, match="pair_rows"):
        ops.disc_tap_eval(c, scale, shift, out, None, 2, torch.empty(2, device=DEV))
    with pytest.raises(_lib.VaePlayHipError, match="dist"):
        ops.disc_tap_eval(c, scale, shift, out, None, 1, None)
    with pytest.raises(_lib.VaePlayHipError, match="nothing to write"):
        ops.disc_tap_eval(c, scale, shift, None, None, 0, None)
    with pytest.raises(_lib.VaePlayHipError, match="multiple of 32"):
        ops.disc_tap_eval(torch.zeros(2, 64, 48, device=DEV), scale, shift, out, None, 0, None)


# ---- K3: the head ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H", [(1, 512), (5, 512), (64, 512), (3, 8)])
def test_head_against_fp64(n, H):
    from vae_play_amd import ops
    g = gen(200 + n + H)
    h = torch.randn(n, H, generator=g)
    scale, shift = torch.rand(H, generator=g) + 0.5, torch.randn(H, generator=g) * 0.3
    scale[::5] *= -1.0
    w = torch.randn(H, generator=g) / H ** 0.5
    bias = torch.tensor([0.37])
    D = torch.float64
    # logits planted near +-30 next to the ordinary ones: the row's activation is a multiple of the weights of the wanted sign (zero
    # on the other columns), a = gain * max(+-w, 0), so that sum a w = +-gain * sum of those w^2; h = (a - t) / s undoes the BatchNorm
    plant = {0: 30.0, n - 1: -30.0} if n > 1 else {0: 30.0}
    for r, target in plant.items():
        pos = (w if target > 0 else -w).clamp(min=0.0)
        gain = abs(target - float(bias)) / float((pos.to(D) * w.to(D).abs()).sum())
        h[r] = (gain * pos - shift) / scale
    # the activation as the kernel rounds it -- ONE rounding of h s + t, formed exactly in fp64's 53 bits -- then everything in fp64
    a = (h.to(D) * scale.to(D) + shift.to(D)).clamp(min=0.0).float()
    logit = a.to(D) @ w.to(D) + bias.to(D)
    print(f"head n{n} H{H}: logits {logit.min().item():.2f} .. {logit.max().item():.2f}")
    p_ref, _, _ = small_ref.gan_head(logit.repeat(3), n, 1.0)
    p_ref = p_ref[:n]
    q_ref = 1.0 / (1.0 + torch.exp(logit))           # small_ref.gan_head's q
    ref = {"logit": logit, "p": p_ref, "nl_real": -torch.log(p_ref + 1e-3), "nl_fake": -torch.log(q_ref + 1e-3)}
    hd, sd, td, wd, bd = (t.to(DEV) for t in (h, scale, shift, w, bias))
    runs = []
    for _ in range(2):
        G = Guards()
        out = {k: G.out(k, n) for k in ref}
        ops.disc_head_eval(hd, sd, td, wd, bd, out["logit"], out["p"], out["nl_real"], out["nl_fake"])
        G.check()
        runs.append(out)
    for k in ref:
        scalar_close(runs[0][k], ref[k], f"head n{n} H{H} {k}")         # each element relative to itself
        assert same_bits(runs[0][k], runs[1][k]), f"{k}: two runs differ"
    # every output is optional
    G = Guards()
    only_p = G.out("p", n)
    ops.disc_head_eval(hd, sd, td, wd, bd, None, only_p, None, None)
    G.check()
    assert same_bits(only_p, runs[0]["p"])


def test_head_saturated_logits_keep_their_digits():
    """logits planted at +-30 exactly (H = 1, activation 1): p and 1 - p come from sigmoid_pair, not from 1.f - p"""
    from vae_play_amd import ops
    logit = torch.tensor([30.0, -30.0, 0.0, 2.5, -7.0], dtype=torch.float64)
    n = logit.numel()
    h = logit.float().view(n, 1).to(DEV)
    one, zero = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    G = Guards()
    out = {k: G.out(k, n) for k in ("logit", "p", "nl_real", "nl_fake")}
    # relu would clip the negative rows: carry the sign in the weight instead (h = |logit|, w = 1 for +, rows run one at a time)
    for i in range(n):
        sgn = torch.tensor([1.0 if logit[i] >= 0 else -1.0], device=DEV)
        ops.disc_head_eval(h[i:i + 1].abs().contiguous(), one, zero, sgn, zero, out["logit"][i:i + 1], out["p"][i:i + 1],
                           out["nl_real"][i:i + 1], out["nl_fake"][i:i + 1])
    G.check()
    p = 1.0 / (1.0 + torch.exp(-logit))
    q = 1.0 / (1.0 + torch.exp(logit))
    scalar_close(out["logit"], logit, "planted logit", tol=0.0)
    scalar_close(out["p"], p, "planted p")
    scalar_close(out["nl_real"], -torch.log(p + 1e-3), "planted nl_real")
    scalar_close(out["nl_fake"], -torch.log(q + 1e-3), "planted nl_fake")


# ---- K4: the fold ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(1, 32, 64), (3, 64, 128), (3, 512, 8), (2, 32, 64)])
def test_lin_fold_against_fp64(M, N, K):
    from vae_play_amd import ops
    g = gen(300 + M + N + K)
    w_out, b_out = torch.randn(M, N, generator=g) / N ** 0.5, torch.randn(M, generator=g) * 0.1
    w, b = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g) * 0.1
    G = Guards()
    w_new, b_new = G.out("w_new", M, K), G.out("b_new", M)
    ops.lin_fold(w_out.to(DEV), b_out.to(DEV), w.to(DEV), b.to(DEV), w_new, b_new)
    G.check()
    tensor_close(w_new.cpu(), w_out.double() @ w.double(), f"lin_fold {M}x{N}x{K} W")
    tensor_close(b_new.cpu(), w_out.double() @ b.double() + b_out.double(), f"lin_fold {M}x{N}x{K} b")
