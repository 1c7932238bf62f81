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
