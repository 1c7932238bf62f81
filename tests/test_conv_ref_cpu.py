"""The fp64 direct-sum reference of tests/conv_ref.py against torch's own float64 convolutions at small shapes (CPU only), and the
negative controls that show why the GPU tests compare with it: a gather with transposed taps and a scatter with the wrong phase
mapping satisfy the bilinear-form identities of tests/test_gpu_properties.py -- both are consistent permutations -- yet the
direct-sum check rejects them by a wide margin."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R

TAU_MAX = 1e-4     # the loosest tolerance the GPU tests apply (f16x2, two products)


def _operands(B, Cb, Cs, Hs, seed):
    g = torch.Generator().manual_seed(seed)
    big = torch.randn(B, Cb, 2 * Hs, 2 * Hs, generator=g, dtype=torch.float64).contiguous(memory_format=torch.channels_last)
    small = torch.randn(B, Cs, Hs, Hs, generator=g, dtype=torch.float64).contiguous(memory_format=torch.channels_last)
    w = torch.randn(Cs, Cb, 5, 5, generator=g, dtype=torch.float64) * 0.05
    return big, small, w


def _torch_families(big, small, w):
    gather = F.conv2d(big, w, stride=2, padding=2)
    scatter = F.conv_transpose2d(small, w, stride=2, padding=2, output_padding=1)
    wv = w.clone().requires_grad_(True)
    F.conv2d(big, wv, stride=2, padding=2).backward(small)
    return gather, scatter, wv.grad


SHAPES = [(2, 8, 16, 8), (3, 16, 8, 6), (1, 4, 4, 4)]      # (B, Cb, Cs, Hs); Hs = 4 makes the sampled rows overlap


@pytest.mark.parametrize("B,Cb,Cs,Hs", SHAPES)
def test_direct_sums_match_torch_float64(B, Cb, Cs, Hs):
    big, small, w = _operands(B, Cb, Cs, Hs, seed=B * 100 + Cb)
    gather, scatter, dw = _torch_families(big, small, w)
    assert gather.shape == small.shape and scatter.shape == big.shape

    gp = R.gather_points(B, Hs, seed=1)
    r, A = R.gather_ref(big, w, gp)
    assert r.shape == (len(gp), Cs) and (A >= r.abs()).all()
    assert R.worst(R.take(gather, gp), r, A)[0] <= 1e-13

    sp = R.scatter_points(B, 2 * Hs, seed=1)
    assert {(y % 2, x % 2) for _, y, x in sp} == {(0, 0), (0, 1), (1, 0), (1, 1)}, "every phase is sampled"
    r, A = R.scatter_ref(small, w, sp)
    assert r.shape == (len(sp), Cb) and (A >= r.abs()).all()
    assert R.worst(R.take(scatter, sp), r, A)[0] <= 1e-13

    cs, cb = R.edge_channels(Cs), R.edge_channels(Cb)
    r, A = R.wgrad_ref(big, small, cs, cb)
    assert R.worst(dw[cs][:, cb], r, A)[0] <= 1e-13


def test_sample_sets():
    assert R.edge_channels(1024) == [0, 63, 64, 127, 128, 1023]
    assert R.edge_channels(64) == [0, 63]
    assert R.edge_channels(128) == [0, 63, 64, 127]
    assert sorted({h for _, h, _ in R.gather_points(32, 8, 0)}) == [0, 1, 4, 6, 7]
    assert sorted({y for _, y, _ in R.scatter_points(32, 16, 0)}) == [0, 1, 2, 3, 8, 9, 14, 15]
    assert {b for b, _, _ in R.gather_points(32, 8, 0)} >= {0, 31}
    sp = R.scatter_points(2, 8, 0)
    terms = R.scatter_terms(sp, 4, 4, 5)
    ones = F.conv_transpose2d(torch.ones(2, 5, 4, 4, dtype=torch.float64), torch.ones(5, 1, 5, 5, dtype=torch.float64), stride=2,
                              padding=2, output_padding=1)
    assert terms.tolist() == [int(ones[b, 0, y, x].item()) for b, y, x in sp]     # from 9 taps inside down to 1 at the far corner
    assert terms.min().item() == 5 and terms.max().item() == 45


@pytest.mark.parametrize("B,Cb,Cs,Hs", SHAPES[:2])
def test_direct_sum_check_rejects_transposed_taps_and_wrong_phase(B, Cb, Cs, Hs):
    """A transposed (r, q) and a swapped stride-2 phase keep gather, scatter and the weight gradient one bilinear form when all three
    families share the mistake; the direct sum sees them at once: far above the loosest tolerance of the GPU tests."""
    big, small, w = _operands(B, Cb, Cs, Hs, seed=7 + Cs)
    wt = w.transpose(2, 3)
    wrong = F.conv2d(big, wt, stride=2, padding=2)
    wrong_t = F.conv_transpose2d(small, wt, stride=2, padding=2, output_padding=1)
    # the mistake, made in both families, still passes the adjointness test of tests/test_gpu_properties.py
    lhs, rhs = (wrong * small).sum().item(), (big * wrong_t).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * (wrong.norm() * small.norm()).item()

    gp = R.gather_points(B, Hs, seed=2)
    r, A = R.gather_ref(big, w, gp)
    assert R.worst(R.take(wrong, gp), r, A)[0] > 100 * TAU_MAX, "transposed taps must fail the gather check"

    sp = R.scatter_points(B, 2 * Hs, seed=2)
    r, A = R.scatter_ref(small, w, sp)
    assert R.worst(R.take(wrong_t, sp), r, A)[0] > 100 * TAU_MAX, "transposed taps must fail the scatter check"
    scatter = F.conv_transpose2d(small, w, stride=2, padding=2, output_padding=1)
    flip = torch.arange(2 * Hs) ^ 1                                          # row y takes the result of row y ^ 1: phases swapped
    assert R.worst(R.take(scatter[:, :, flip], sp), r, A)[0] > 100 * TAU_MAX, "a swapped phase must fail the scatter check"

    cs, cb = R.edge_channels(Cs), R.edge_channels(Cb)
    r, A = R.wgrad_ref(big, small, cs, cb)
    dw = _torch_families(big, small, w)[2]
    assert R.worst(dw[cs][:, cb], r, A)[0] <= 1e-13
    assert R.worst(dw.transpose(2, 3)[cs][:, cb], r, A)[0] > 100 * TAU_MAX, "transposed taps must fail the weight-gradient check"


# ---- k x k geometries: ks in {1, 3, 5}, stride 1 | 2, padding (ks - 1) // 2, any big side (tests/test_gpu_conv_direct_kxk.py) ----------
KXK_SIDES = {"even": (8, 8), "odd": (9, 9), "nonsquare": (7, 10)}
KXK_CHANNELS = [(1, 4), (3, 2), (10, 18), (34, 16)]        # (Cb, Cs): 1-4 channels, counts the front end pads to 8, a 32-tile edge


def _kxk_operands(B, Cb, Cs, Hb, Wb, ks, stride, seed):
    g = torch.Generator().manual_seed(seed)
    Hs, Ws = R.out_size(Hb, ks, stride), R.out_size(Wb, ks, stride)
    big = torch.randn(B, Cb, Hb, Wb, generator=g, dtype=torch.float64).contiguous(memory_format=torch.channels_last)
    small = torch.randn(B, Cs, Hs, Ws, generator=g, dtype=torch.float64).contiguous(memory_format=torch.channels_last)
    w = torch.randn(Cs, Cb, ks, ks, generator=g, dtype=torch.float64) * 0.1
    return big, small, w


def _kxk_torch(big, small, w, stride):
    """torch's float64 gather (conv2d), scatter (conv_transpose2d with the output_padding that gives Hb x Wb) and weight gradient"""
    ks = w.shape[-1]
    p = R.pad_of(ks)
    Hb, Wb = big.shape[2:]
    Hs, Ws = small.shape[2:]
    op = (Hb - ((Hs - 1) * stride - 2 * p + ks), Wb - ((Ws - 1) * stride - 2 * p + ks))
    assert 0 <= min(op) and max(op) < stride
    gather = F.conv2d(big, w, stride=stride, padding=p)
    scatter = F.conv_transpose2d(small, w, stride=stride, padding=p, output_padding=op)
    dw = torch.nn.grad.conv2d_weight(big, w.shape, small, stride=stride, padding=p)
    return gather, scatter, dw


def _kxk_case_id(ks, stride, side, ch):
    return f"k{ks}s{stride}-{side}-cb{ch[0]}cs{ch[1]}"


KXK_CASES = [(ks, s, side, ch) for ks in (1, 3, 5) for s in (1, 2) for side in KXK_SIDES for ch in KXK_CHANNELS]


@pytest.mark.parametrize("ks,stride,side,ch", KXK_CASES, ids=[_kxk_case_id(*c) for c in KXK_CASES])
def test_kxk_direct_sums_match_torch_float64(ks, stride, side, ch):
    (Hb, Wb), (Cb, Cs), B = KXK_SIDES[side], ch, 2
    big, small, w = _kxk_operands(B, Cb, Cs, Hb, Wb, ks, stride, seed=ks * 1000 + stride * 100 + Cb)
    Hs, Ws = small.shape[2:]
    gather, scatter, dw = _kxk_torch(big, small, w, stride)
    assert gather.shape == small.shape and scatter.shape == big.shape

    gp = R.gather_points(B, Hs, seed=1, Ws=Ws)
    r, A, K = R.gather_ref(big, w, gp, stride, terms=True)
    assert r.shape == K.shape == (len(gp), Cs) and (A >= r.abs()).all()
    assert R.worst(R.take(gather, gp), r, A)[0] <= 1e-13
    ones = F.conv2d(torch.ones(B, Cb, Hb, Wb, dtype=torch.float64), torch.ones(1, Cb, ks, ks, dtype=torch.float64), stride=stride,
                    padding=R.pad_of(ks))
    assert K[:, 0].tolist() == [int(ones[b, 0, h, x].item()) for b, h, x in gp], "gather term counts"

    sp = R.scatter_points(B, Hb, seed=1, Wb=Wb)
    if stride == 2:
        assert {(y % 2, x % 2) for _, y, x in sp} == {(0, 0), (0, 1), (1, 0), (1, 1)}, "every phase is sampled"
    assert {Hb - 1, Hb - 2} <= {y for _, y, _ in sp} and {Wb - 1, Wb - 2} <= {x for _, _, x in sp}, "both last lines are sampled"
    r, A, K = R.scatter_ref(small, w, sp, stride, terms=True)
    assert r.shape == K.shape == (len(sp), Cb) and (A >= r.abs()).all()
    assert R.worst(R.take(scatter, sp), r, A)[0] <= 1e-13
    ones_t = F.conv_transpose2d(torch.ones(B, Cs, Hs, Ws, dtype=torch.float64), torch.ones(Cs, 1, ks, ks, dtype=torch.float64),
                                stride=stride, padding=R.pad_of(ks), output_padding=(Hb - (Hs - 1) * stride + 2 * R.pad_of(ks) - ks,
                                                                                      Wb - (Ws - 1) * stride + 2 * R.pad_of(ks) - ks))
    counts = [int(ones_t[b, 0, y, x].item()) for b, y, x in sp]
    assert K[:, 0].tolist() == counts == R.scatter_terms(sp, Hs, Ws, Cs, ks, stride).tolist(), "scatter term counts"

    cs, cb = R.tile_channels(Cs), R.tile_channels(Cb)
    r, A, K = R.wgrad_ref(big, small, cs, cb, ks, stride, terms=True)
    assert R.worst(dw[cs][:, cb], r, A)[0] <= 1e-13
    cnt = torch.nn.grad.conv2d_weight(torch.ones(B, 1, Hb, Wb, dtype=torch.float64), (1, 1, ks, ks), torch.ones(B, 1, Hs, Ws, dtype=torch.float64),
                                      stride=stride, padding=R.pad_of(ks))
    assert torch.equal(K[0, 0].double(), cnt[0, 0]), "weight-gradient term counts"


def test_kxk_sample_sets_and_default_geometry():
    assert R.out_size(9, 3, 2) == 5 and R.out_size(8, 3, 2) == 4 and R.out_size(9, 1, 2) == 5 and R.out_size(255, 5, 2) == 128
    assert R.tile_channels(34) == [0, 7, 8, 15, 16, 31, 32, 33]      # 33: the last real channel of a count padded to 40
    assert R.tile_channels(2) == [0, 1] and R.tile_channels(1) == [0]
    assert R.tile_channels(256) == [0, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255]
    assert sorted({y for _, y, _ in R.scatter_points(2, 9, 0)}) == [0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert sorted({y for _, y, _ in R.scatter_points(2, 33, 0)}) == [0, 1, 2, 3, 16, 17, 30, 31, 32]
    assert sorted({x for _, _, x in R.gather_points(2, 5, 0, Ws=9)}) == [0, 1, 4, 7, 8]
    # the 5x5 stride-2 defaults are the old functions' (tests/test_gpu_properties.py, tests/test_gpu_wgrad_budget.py call them so)
    big, small, w = _operands(2, 8, 16, 4, seed=3)
    gp, sp = R.gather_points(2, 4, 1), R.scatter_points(2, 8, 1)
    for got, want in ((R.gather_ref(big, w, gp), R.gather_ref(big, w, gp, 2)), (R.scatter_ref(small, w, sp), R.scatter_ref(small, w, sp, 2)),
                      (R.wgrad_ref(big, small, [0, 15], [0, 7]), R.wgrad_ref(big, small, [0, 15], [0, 7], 5, 2))):
        assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_tau_from_the_arithmetic():
    t = lambda K, m: R.tau(K, m).item()
    assert t(392, "f32") == pytest.approx(10 * 1.6 * 2.0 ** -24) and t(392, "f32") <= 1e-6
    assert t(392, "bf16x3") == pytest.approx(10 * (1.6 * 2.0 ** -24 + 2 * 2.0 ** -17 * 1.57 / 392 ** 0.5))
    assert t(1, "bf16x3") == pytest.approx(10 * (2.0 ** -24 + 2 * 2.0 ** -17)), "K = 1: the deterministic worst case"
    assert t(4, "small3") == t(4, "f32") and t(16, "f16x2/2 declared") == t(16, "f16x2/3")
    assert t(4, "bf16x3") > t(16, "bf16x3") > t(392, "bf16x3")


def _adjoint_and_bilinear(big, small, w, stride, gather, scatter, dw):
    """the identities of tests/test_gpu_properties*.py: <conv(x), y> = <x, conv^T(y)> = <w, wgrad(x, y)>, to 3e-6 * |conv(x)| |y|"""
    lhs = (gather * small).sum().item()
    scale = (gather.norm() * small.norm()).item()
    return abs(lhs - (big * scatter).sum().item()) <= 3e-6 * scale and abs(lhs - (w * dw).sum().item()) <= 3e-6 * scale


def _margins(big, small, w, stride, fams, seed):
    """worst |out - r| / (tau_bf16x3(K) * A) of the three families' outputs `fams` (gather, scatter, wgrad) against the direct sums
    of the true weight w"""
    B, Cb, Hb, Wb = big.shape
    _, Cs, Hs, Ws = small.shape
    gp, sp = R.gather_points(B, Hs, seed, Ws=Ws), R.scatter_points(B, Hb, seed, Wb=Wb)
    cs, cb = R.tile_channels(Cs), R.tile_channels(Cb)
    out = {}
    r, A, K = R.gather_ref(big, w, gp, stride, terms=True)
    out["gather"] = R.worst_scaled(R.take(fams[0], gp), r, A, R.tau(K, "bf16x3"))[0]
    r, A, K = R.scatter_ref(small, w, sp, stride, terms=True)
    out["scatter"] = R.worst_scaled(R.take(fams[1], sp), r, A, R.tau(K, "bf16x3"))[0]
    r, A, K = R.wgrad_ref(big, small, cs, cb, w.shape[-1], stride, terms=True)
    out["wgrad"] = R.worst_scaled(fams[2][cs][:, cb], r, A, R.tau(K, "bf16x3"))[0]
    return out


CONTROL_CASES = [(s, side) for s in (1, 2) for side in KXK_SIDES]


@pytest.mark.parametrize("stride,side", CONTROL_CASES, ids=[f"k3s{s}-{side}" for s, side in CONTROL_CASES])
@pytest.mark.parametrize("mistake", ["transposed_taps", "mirrored_phase_map", "channels_swapped_in_tile"])
def test_kxk_direct_sum_check_rejects_consistent_mistakes(mistake, stride, side):
    """Three mistakes a 3x3 kernel could make in all three families at once -- taps transposed; the stride-2 phase map of the pad-1
    scatter mirrored (an odd big line takes tap 0 from small line h and tap 2 from h + 1 instead of 2 and 0 -- on both axes the
    flipped kernel); big-side channels 0 and 7 swapped inside the first 8-wide tile -- keep gather, scatter and weight gradient one
    bilinear form, so they pass the identities of tests/test_gpu_properties*.py.  The direct sums reject each by more than 100 tau
    of the loosest k x k mode (bf16x3) in every family."""
    (Hb, Wb), B, Cb, Cs = KXK_SIDES[side], 2, 16, 8
    big, small, w = _kxk_operands(B, Cb, Cs, Hb, Wb, 3, stride, seed=40 + stride)
    perm = list(range(Cb))
    perm[0], perm[7] = 7, 0
    mis = {"transposed_taps": lambda t: t.transpose(2, 3), "mirrored_phase_map": lambda t: t.flip(2, 3),
           "channels_swapped_in_tile": lambda t: t[:, perm]}[mistake]          # each its own adjoint on the weight space
    gather, scatter, dw = _kxk_torch(big, small, mis(w), stride)
    fams = (gather, scatter, mis(dw))          # the weight gradient of the mistaken form <conv(x, mis(w)), y> is mis(wgrad(x, y))
    assert _adjoint_and_bilinear(big, small, w, stride, *fams), "the mistake must keep the bilinear-form identities"
    assert max(_margins(big, small, w, stride, _kxk_torch(big, small, w, stride), seed=5).values()) <= 1e-6, "the correct operation passes"
    margins = _margins(big, small, w, stride, fams, seed=5)
    print(f"{mistake} k3s{stride} {side}: err / tau " + ", ".join(f"{k} {v:.0f}" for k, v in margins.items()))
    for fam, m in margins.items():
        assert m > 100, f"{mistake}: the {fam} check passes it (err / tau = {m:.1f}, need > 100)"
