"""The affine-activation epilogue of the 5x5 implicit-GEMM convolutions (vp_conv5_{gather,scatter}_affine_{bf16x3,f32}) at every
launch shape the inference plans fuse at 128x128x3 batch 32 and 64x64x3 batch 128, against fp64 direct sums (tests/conv_ref.py)
followed by the fp64 affine map and ReLU at sampled output pixels (all channels of each).

Bound, from the arithmetic, fixed before any measurement.  With r, A, K of the sample (conv_ref) the convolution part keeps
|acc - r| <= tau(K, mode) A.  The epilogue is v = relu(fma(acc, s, t)) -- ONE fma, so one fp32 rounding; the bound allows two, as
for a multiply and an add -- and ReLU is 1-Lipschitz:
    |v - relu(r s + t)| <= |s| tau(K, mode) A + SAFETY 2 2^-24 (|r s| + |t|)
and the recombined planes hi + lo, which keep 16 significant bits (csrc/split.h), that plus 2^-16 |v|.

Bit equalities that must hold: with both outputs requested from one launch the planes are split.h's split (ops.split_f32) of that
launch's own fp32 output; the fp32 output is the same whether or not planes are requested; the planes are the same whether or not
the fp32 output is requested.  The optional identity against the un-fused entry point (affine applied by an elementwise op to its
fp32 output) is NOT asserted: the un-fused entry points dispatch other kernels (halo, pipelined, 16x16x32 MFMA form) with another
summation order at several of these shapes, and the epilogue is one fma where an elementwise multiply and add rounds twice."""
import pytest
import torch

from tests import conv_ref as R

pytestmark = pytest.mark.gpu

# (B, Hs, Cin, Cout): small-side extent Hs, stride 2
GATHER = {"bf16x3": [(32, 32, 64, 128), (32, 16, 128, 256), (128, 16, 64, 128), (128, 8, 128, 256)],
          "f32": [(32, 32, 64, 128), (128, 16, 64, 128)]}
SCATTER = [(32, 8, 512, 512), (32, 16, 512, 256), (32, 32, 256, 128), (32, 64, 128, 64),
           (128, 8, 256, 256), (128, 16, 256, 128), (128, 32, 128, 64)]
CASES = [(0, prec, s) for prec in ("bf16x3", "f32") for s in GATHER[prec]] + [(1, prec, s) for prec in ("bf16x3", "f32") for s in SCATTER]


def _rows_to_points(family, rows, Hs):
    """tile rows m = (b, h, x) of the flattened small side -> sampled output pixels: the pixel itself (gather) or the four
    pixels (2h + ph, 2x + pw) it owns in the four phases (scatter)"""
    pts = []
    for m in rows:
        b, rem = divmod(m, Hs * Hs)
        h, x = divmod(rem, Hs)
        pts += [(b, h, x)] if family == 0 else [(b, 2 * h + ph, 2 * x + pw) for ph in (0, 1) for pw in (0, 1)]
    return pts


@pytest.mark.parametrize("family,prec,shape", CASES, ids=[f"{'gs'[f]}-{p}-{'x'.join(map(str, s))}" for f, p, s in CASES])
def test_affine_epilogue_vs_fp64_direct_sums(family, prec, shape):
    from vae_play_amd import ops
    B, Hs, Cin, Cout = shape
    Cbig, Csmall = (Cin, Cout) if family == 0 else (Cout, Cin)
    assert ops.conv5_affine_supported(family, prec, B, Hs, Hs, Cbig, Csmall, 2), "a launch shape the plans fuse must be supported"
    gen = torch.Generator(device="cuda").manual_seed(1234 + 7 * family + Hs + Cin)
    Hin = 2 * Hs if family == 0 else Hs
    a = torch.randn((B, Cin, Hin, Hin), device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    if family == 0:
        w = torch.randn((Cout, Cin, 5, 5), device="cuda", generator=gen) / (25 * Cin) ** 0.5        # Conv2d weight [Cs][Cb]
    else:
        w = torch.randn((Cin, Cout, 5, 5), device="cuda", generator=gen) / (6.25 * Cin) ** 0.5      # ConvTranspose2d weight [Cs][Cb]
    scale = torch.empty(Cout, device="cuda").uniform_(0.5, 1.5, generator=gen)
    scale[1::3] *= -1.0                                                                             # (a BatchNorm's gamma may be negative)
    shift = torch.randn(Cout, device="cuda", generator=gen) * 0.2
    if prec == "bf16x3":
        a_in = ops.split_f32(a)
        wp = ops.pack_w5_split(w, family == 0, family == 1)[family]
    else:
        a_in = a
        wp = ops.pack_w5(w, family == 0, family == 1)[family]
    both = prec == "bf16x3"
    out, planes = ops.conv5_affine(family, prec, a_in, a.shape, wp, Cout, scale, shift, 2, ops.ACT_RELU, True, both)
    torch.cuda.synchronize()

    # ---- bit equalities ----
    if both:
        assert torch.equal(planes, ops.split_f32(out)), "planes != split.h's split of the launch's own fp32 output"
        only32, _ = ops.conv5_affine(family, prec, a_in, a.shape, wp, Cout, scale, shift, 2, ops.ACT_RELU, True, False)
        assert torch.equal(only32, out), "the fp32 output depends on whether planes are requested"
        _, only_s = ops.conv5_affine(family, prec, a_in, a.shape, wp, Cout, scale, shift, 2, ops.ACT_RELU, False, True)
        assert torch.equal(only_s, planes), "the planes depend on whether the fp32 output is requested"
    again, _ = ops.conv5_affine(family, prec, a_in, a.shape, wp, Cout, scale, shift, 2, ops.ACT_RELU, True, False)
    assert torch.equal(again, out), "two launches differ"

    # ---- fp64 direct sums at sampled pixels: borders and middle of the image, first / last tile row, 64- and 128-row tile boundaries ----
    M = B * Hs * Hs
    rows = sorted({m for m in (0, 1, 63, 64, 127, 128, 255, 256, M // 2 - 1, M // 2, M - 129, M - 128, M - 65, M - 64, M - 1) if 0 <= m < M})
    Ho = Hs if family == 0 else 2 * Hs
    pts = (R.gather_points(B, Hs, 5) if family == 0 else R.scatter_points(B, Ho, 5)) + _rows_to_points(family, rows, Hs)
    pts = sorted(set(pts))
    r, A, K = (R.gather_ref if family == 0 else R.scatter_ref)(a, w, pts, terms=True)
    s64, t64 = scale.double()[None, :], shift.double()[None, :]
    ref = torch.relu(r * s64 + t64)
    bound = s64.abs() * R.tau(K, prec).to(r.device) * A + R.SAFETY * 2 * 2.0 ** -24 * ((r * s64).abs() + t64.abs())
    got = R.take(out, pts)
    err = (got - ref).abs()
    worst = (err / bound).max().item()
    print(f"affine {('gather', 'scatter')[family]} {prec} {shape}: {len(pts)} pixels x {Cout} channels, worst |v - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, f"fp32 output outside the bound: {worst:.3f} x"
    if both:
        rec = ops.unsplit(planes).view(B, Ho, Ho, Cout).permute(0, 3, 1, 2)
        gp = R.take(rec, pts)
        worst_p = ((gp - ref).abs() / (bound + 2.0 ** -16 * got.abs())).max().item()
        print(f"   planes hi + lo: worst / bound = {worst_p:.3f}")
        assert worst_p <= 1.0, f"recombined planes outside the bound: {worst_p:.3f} x"
    # ReLU actually cuts: both signs occur among the samples
    assert (ref == 0).any() and (ref > 0).any()


def test_act_none_and_channel_constants_are_per_output_channel():
    """act = none keeps negative values; scale / shift are indexed by the OUTPUT channel (a one-hot scale leaves one channel)"""
    from vae_play_amd import ops
    B, Hs, Cin, Cout = 4, 16, 64, 128
    gen = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randn((B, Cin, 2 * Hs, 2 * Hs), device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    w = torch.randn((Cout, Cin, 5, 5), device="cuda", generator=gen) / 40.0
    wp = ops.pack_w5_split(w, True, False)[0]
    one = torch.ones(Cout, device="cuda")
    zero = torch.zeros(Cout, device="cuda")
    assert ops.conv5_affine_supported(0, "bf16x3", B, Hs, Hs, Cin, Cout, 2)
    plain, _ = ops.conv5_affine(0, "bf16x3", ops.split_f32(a), a.shape, wp, Cout, one, zero, 2, ops.ACT_NONE)
    assert (plain < 0).any()
    hot = zero.clone()
    hot[37] = 2.0
    sh = zero.clone()
    sh[5] = 0.25
    o, _ = ops.conv5_affine(0, "bf16x3", ops.split_f32(a), a.shape, wp, Cout, hot, sh, 2, ops.ACT_NONE)
    expect = torch.zeros_like(plain)
    expect[:, 37] = 2.0 * plain[:, 37]
    expect[:, 5] = 0.25
    assert torch.equal(o, expect)


def test_bn_fold_against_fp64():
    """vp_bn_fold_f32: s = gamma / sqrt(var + eps), t = beta - mean s, rstd = 1 / sqrt(var + eps), each within one fp32 rounding
    (2^-24 relative) of the fp64 value"""
    from vae_play_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(11)
    C, eps = 517, 1e-5
    gamma = torch.empty(C, device="cuda").uniform_(0.5, 1.5, generator=gen)
    beta = torch.randn(C, device="cuda", generator=gen) * 0.2
    mean = torch.randn(C, device="cuda", generator=gen)
    var = torch.empty(C, device="cuda").uniform_(0.01, 4.0, generator=gen)
    scale, shift, rstd = ops.bn_fold(gamma, beta, mean, var, eps)
    e = float(torch.tensor(eps, dtype=torch.float32).double())       # the entry point takes eps as fp32
    r64 = 1.0 / torch.sqrt(var.double() + e)
    s64 = gamma.double() * r64
    t64 = beta.double() - mean.double() * s64
    u = 2.0 ** -24
    assert ((rstd.double() - r64).abs() <= u * r64.abs()).all()
    assert ((scale.double() - s64).abs() <= u * s64.abs()).all()
    assert ((shift.double() - t64).abs() <= u * t64.abs() + 1e-45).all()


def test_error_paths():
    """host-side validation only: nothing here reaches a launch"""
    from vae_play_amd import _lib, ops
    B, Hs, Cin, Cout = 4, 16, 64, 128
    a = torch.zeros((B, Cin, 2 * Hs, 2 * Hs), device="cuda").contiguous(memory_format=torch.channels_last)
    a_s = ops.split_f32(a)
    wp = ops.pack_w5_split(torch.zeros((Cout, Cin, 5, 5), device="cuda"), True, False)[0]
    wp32 = ops.pack_w5(torch.zeros((Cout, Cin, 5, 5), device="cuda"), True, False)[0]
    s = torch.ones(Cout, device="cuda")
    with pytest.raises(_lib.VaePlayHipError, match="both outputs are null"):
        ops.conv5_affine(0, "bf16x3", a_s, a.shape, wp, Cout, s, s, 2, ops.ACT_RELU, False, False)
    with pytest.raises(_lib.VaePlayHipError, match="bf16x3 entry point only"):
        ops.conv5_affine(0, "f32", a, a.shape, wp32, Cout, s, s, 2, ops.ACT_RELU, True, True)
    with pytest.raises(_lib.VaePlayHipError, match="null scale"):
        ops.conv5_affine(0, "bf16x3", a_s, a.shape, wp, Cout, None, s, 2)
    with pytest.raises(_lib.VaePlayHipError, match="none\\|relu"):
        ops.conv5_affine(0, "bf16x3", a_s, a.shape, wp, Cout, s, s, 2, ops.ACT_SIGMOID)
    # a shape whose plain launch splits K (8x8 resolution, few tiles) is refused, and the query says so
    assert not ops.conv5_affine_supported(0, "bf16x3", 4, 8, 8, 256, 512, 2)
    big = ops.split_f32(torch.zeros((4, 256, 16, 16), device="cuda").contiguous(memory_format=torch.channels_last))
    wq = ops.pack_w5_split(torch.zeros((512, 256, 5, 5), device="cuda"), True, False)[0]
    with pytest.raises(_lib.VaePlayHipError, match="vp_conv5_affine_supported"):
        ops.conv5_affine(0, "bf16x3", big, (4, 256, 16, 16), wq, 512, torch.ones(512, device="cuda"), torch.ones(512, device="cuda"), 2)
    assert not ops.conv5_affine_supported(0, "bf16x3", 4, 16, 16, 24, 128, 2)      # contracted side not a multiple of 64
    assert not ops.conv5_affine_supported(1, "f32", 32, 64, 64, 32, 128, 2)        # fewer than 64 output channels
