"""The pointwise and data-movement kernels of csrc/elementwise.hip and the two activation kernels of csrc/bn.hip, each called through
the C ABI on NaN-prefilled, sentinel-guarded outputs (tests/guarded.py).  Data movement (transposes, channel slice, the x channels of
AddCoords, ReLU forward, the ReLU / LReLU derivative masks) must be bit-identical to the fp32 input, vp_add_f32 to torch's fp32
a + b; everything else is held to the fp64 references of tests/small_ref.py at OP_RTOL in rel_err's norm.  The large shapes exceed
grid_for's 2048 blocks x 256 lanes = 524,288 items, so the grid-stride loops take a second trip."""
import pytest
import torch

from tests import small_ref as R
from tests.guarded import Guards, same_bits
from tests.guarded import api as _api, gen as _gen, tensor_close as _tensor
from tests.util import OP_RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = 2 * 524288 + 77


def _cl(nhwc):
    """[B, H, W, C] array -> the logical (B, C, H, W) channels_last tensor the ops wrappers take (same memory)"""
    return nhwc.permute(0, 3, 1, 2)


@pytest.mark.parametrize("n", [1, BIG])
def test_add(n):
    _lib, ops, lib = _api()
    g = _gen(10 + n % 97)
    a_c, b_c = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-3
    a, b = a_c.to(DEV), b_c.to(DEV)
    want = a_c + b_c
    G = Guards()
    out = G.out("out", n)
    _lib.call("vp_add_f32", ops._p(a), ops._p(b), ops._p(out), n, ops._stream())
    G.check()
    assert same_bits(out, want), "out of place: not torch's fp32 a + b"
    G = Guards()
    acc = G.state("a (in place)", a_c)
    _lib.call("vp_add_f32", ops._p(acc), ops._p(b), ops._p(acc), n, ops._stream())
    G.check()
    assert same_bits(acc, want), "in place (out == a): not torch's fp32 a + b"
    assert torch.equal(b.cpu(), b_c), "b was modified"


SLOPE = 0.02
ACTS = [R.ACT_RELU, R.ACT_LRELU, R.ACT_TANH, R.ACT_SIGMOID]


PLANTED = [0.0, -0.0, 20.0, -20.0]


def _act_case(x_c, dy_c, kind):
    _lib, ops, lib = _api()
    n = x_c.numel()
    x, dy = x_c.to(DEV), dy_c.to(DEV)
    slope32 = float(torch.tensor(SLOPE).item())
    tag = f"kind={kind} n={n}" + (f" x={x_c[0].item()!r}" if n == 1 else "")
    G = Guards()
    y = G.out("y", n)
    _lib.call("vp_act_fwd_f32", ops._p(x), ops._p(y), n, kind, SLOPE, ops._stream())
    G.check()
    _tensor(y, R.act(x_c, kind, slope32), f"act_fwd {tag}")
    if kind == R.ACT_RELU:
        assert same_bits(y, torch.where(x_c > 0, x_c, torch.zeros_like(x_c))), "ReLU forward is not a bit copy of x / +0"
    assert same_bits(ops.act_fwd(x, kind, SLOPE), y), "ops.act_fwd differs from the direct call"
    G = Guards()
    dx = G.out("dx", n)
    _lib.call("vp_act_bwd_from_y_f32", ops._p(y), ops._p(dy), ops._p(dx), n, kind, SLOPE, ops._stream())
    G.check()
    y_c = y.cpu()
    _tensor(dx, R.act_bwd_from_y(y_c, dy_c, kind, slope32), f"act_bwd_from_y {tag}")
    if kind in (R.ACT_RELU, R.ACT_LRELU):
        low = 0.0 if kind == R.ACT_RELU else SLOPE
        mask = torch.where(y_c > 0, torch.ones_like(y_c), torch.full_like(y_c, low))
        assert same_bits(dx, dy_c * mask), "the derivative mask is not dy * {1, slope} in one fp32 multiply"
    assert same_bits(ops.act_bwd_from_y(y, dy, kind, SLOPE), dx), "ops.act_bwd_from_y differs from the direct call"


@pytest.mark.parametrize("kind", ACTS)
@pytest.mark.parametrize("n", [1, BIG])
def test_act_fwd_and_bwd_from_y(n, kind):
    """exact zeros of both signs and +-20 are planted in both trips of the loop and in the last block; at n = 1 each of them is the
    one element of a call of its own, after a random one"""
    g = _gen(20 + n % 97 + kind)
    x_c, dy_c = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g)
    if n == 1:
        for v in [x_c[0].item()] + PLANTED:
            _act_case(torch.tensor([v]), dy_c, kind)
        return
    for at in (0, 255, 256, 524288, n - 5):
        x_c[at:at + 4] = torch.tensor(PLANTED)
    _act_case(x_c, dy_c, kind)


@pytest.mark.parametrize("B,C,H,W", [(1, 1, 1, 1), (2, 3, 5, 7), (1, 33, 1, 65), (3, 64, 8, 8), (2, 31, 3, 11)])
def test_transposes(B, C, H, W):
    _lib, ops, lib = _api()
    x_c = torch.randn(B, C, H, W, generator=_gen(30 + C))
    x = x_c.to(DEV)
    G = Guards()
    nhwc = G.out("nhwc", B, H, W, C)
    _lib.call("vp_nchw_to_nhwc_f32", ops._p(x), ops._p(nhwc), B, C, H, W, ops._stream())
    G.check()
    assert same_bits(nhwc, R.nchw_to_nhwc(x_c).float()), "nchw -> nhwc is not the permutation"
    # the other direction on an independent draw, then the round trip
    z_c = torch.randn(B, H, W, C, generator=_gen(31 + C))
    z = z_c.to(DEV)
    G = Guards()
    nchw, back = G.out("nchw", B, C, H, W), G.out("round trip", B, C, H, W)
    _lib.call("vp_nhwc_to_nchw_f32", ops._p(z), ops._p(nchw), B, C, H, W, ops._stream())
    _lib.call("vp_nhwc_to_nchw_f32", ops._p(nhwc), ops._p(back), B, C, H, W, ops._stream())
    G.check()
    assert same_bits(nchw, R.nhwc_to_nchw(z_c).float()), "nhwc -> nchw is not the permutation"
    assert same_bits(back, x_c), "the round trip is not the identity"
    w1 = ops.nchw_to_nhwc(x)
    assert w1.shape == (B, C, H, W) and same_bits(w1.permute(0, 2, 3, 1).contiguous(), nhwc), "ops.nchw_to_nhwc differs"
    w2 = ops.nhwc_to_nchw(_cl(z))
    assert w2.is_contiguous() and same_bits(w2, nchw), "ops.nhwc_to_nchw differs from the direct call"


UP_SHAPES = [(1, 1, 1, 1), (2, 3, 1, 5), (1, 2, 4, 1), (2, 5, 7, 9), (2, 5, 120, 113), (2, 5, 240, 222)]


@pytest.mark.parametrize("B,C,H,W", UP_SHAPES)
def test_upsample2x_bilinear(B, C, H, W):
    """(2, 5, 120, 113): 4 B H W C = 542,400 forward items; (2, 5, 240, 222): B H W C = 532,800 backward items"""
    _lib, ops, lib = _api()
    g = _gen(40 + H)
    x_c, dy_c = torch.randn(B, H, W, C, generator=g), torch.randn(B, 2 * H, 2 * W, C, generator=g)
    x, dy = x_c.to(DEV), dy_c.to(DEV)
    G = Guards()
    y, dx = G.out("y", B, 2 * H, 2 * W, C), G.out("dx", B, H, W, C)
    _lib.call("vp_upsample2x_bilinear_fwd_f32", ops._p(x), ops._p(y), B, H, W, C, ops._stream())
    _lib.call("vp_upsample2x_bilinear_bwd_f32", ops._p(dy), ops._p(dx), B, H, W, C, ops._stream())
    G.check()
    _tensor(y, R.upsample2x_fwd(x_c), f"upsample2x fwd {(B, C, H, W)}")
    _tensor(dx, R.upsample2x_bwd(dy_c), f"upsample2x bwd {(B, C, H, W)}")
    # <up(x), dy> == <x, up^T(dy)> on the kernels' own outputs, summed in fp64: each side carries the fp32 rounding of its kernel,
    # at most OP_RTOL of the sum of the magnitudes of the terms
    y64, dx64 = y.double().cpu(), dx.double().cpu()
    lhs, rhs = (y64 * dy_c.double()).sum().item(), (x_c.double() * dx64).sum().item()
    scale = (y64.abs() * dy_c.double().abs()).sum().item()
    assert abs(lhs - rhs) <= OP_RTOL * scale, f"adjoint identity: {lhs!r} vs {rhs!r} (scale {scale:.3e})"
    wy = ops.upsample2x_fwd(_cl(x))
    assert wy.shape == (B, C, 2 * H, 2 * W) and same_bits(wy.permute(0, 2, 3, 1).contiguous(), y), "ops.upsample2x_fwd differs"
    wdx = ops.upsample2x_bwd(_cl(dy))
    assert wdx.shape == (B, C, H, W) and same_bits(wdx.permute(0, 2, 3, 1).contiguous(), dx), "ops.upsample2x_bwd differs"


COORD_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 4), (2, 90, 97, 30)]


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("B,H,W,C", COORD_SHAPES)
def test_add_coords(B, H, W, C, normalize):
    _lib, ops, lib = _api()
    x_c = torch.randn(B, H, W, C, generator=_gen(50 + H))
    x = x_c.to(DEV)
    G = Guards()
    out = G.out("out", B, H, W, C + 2)
    _lib.call("vp_add_coords_f32", ops._p(x), ops._p(out), B, H, W, C, normalize, ops._stream())
    G.check()
    assert same_bits(out[..., :C].contiguous(), x_c), "the x channels are not a bit copy"
    ref = R.add_coords(x_c, bool(normalize))
    _tensor(out[..., C:], ref[..., C:], f"add_coords coordinates {(B, H, W, C)} normalize={normalize}")
    _tensor(out, ref, f"add_coords {(B, H, W, C)} normalize={normalize}")
    w = ops.add_coords(_cl(x), bool(normalize))
    assert w.shape == (B, C + 2, H, W) and same_bits(w.permute(0, 2, 3, 1).contiguous(), out), "ops.add_coords differs"


@pytest.mark.parametrize("B,H,W,C", COORD_SHAPES)
def test_slice_channels(B, H, W, C):
    """the gradient of AddCoords: Cin = C + 2 channels in (558,720 items at the last shape when all are kept)"""
    _lib, ops, lib = _api()
    Cin = C + 2
    x_c = torch.randn(B, H, W, Cin, generator=_gen(60 + H))
    x = x_c.to(DEV)
    for Cout in (Cin, Cin - 2, 1):
        G = Guards()
        out = G.out("out", B, H, W, Cout)
        _lib.call("vp_slice_channels_f32", ops._p(x), ops._p(out), B * H * W, Cin, Cout, ops._stream())
        G.check()
        assert same_bits(out, R.slice_channels(x_c, Cout).float()), f"Cout={Cout}: not a bit copy of the first channels"
    w = ops.slice_channels(_cl(x), 1)
    assert w.shape == (B, 1, H, W) and same_bits(w.permute(0, 2, 3, 1).contiguous(), out), "ops.slice_channels differs"


@pytest.mark.parametrize("B,HW,C", [(2, 1, 3), (1, 3, 64), (3, 5, 130), (2, 4100, 65)])
def test_global_avgpool(B, HW, C):
    """pixel lanes idle (HW < 4) | one full 64-channel group | a ragged third group | B HW C = 533,000 backward items"""
    _lib, ops, lib = _api()
    g = _gen(70 + C)
    x_c, dy_c = torch.randn(B, HW, C, generator=g) + 0.5, torch.randn(B, C, generator=g)
    x, dy = x_c.to(DEV), dy_c.to(DEV)
    runs = []
    for _ in range(2):
        G = Guards()
        out = G.out("out", B, C)
        _lib.call("vp_global_avgpool_fwd_f32", ops._p(x), ops._p(out), B, HW, C, ops._stream())
        G.check()
        runs.append(out.clone())
    _tensor(runs[0], R.global_avgpool_fwd(x_c), f"global_avgpool fwd {(B, HW, C)}")
    assert same_bits(runs[0], runs[1]), "two runs differ"
    G = Guards()
    dx = G.out("dx", B, HW, C)
    _lib.call("vp_global_avgpool_bwd_f32", ops._p(dy), ops._p(dx), B, HW, C, ops._stream())
    G.check()
    _tensor(dx, R.global_avgpool_bwd(dy_c, HW), f"global_avgpool bwd {(B, HW, C)}")
    x4 = x.view(B, HW, 1, C).permute(0, 3, 1, 2)
    assert same_bits(ops.global_avgpool_fwd(x4), runs[0]), "ops.global_avgpool_fwd differs from the direct call"
    wdx = ops.global_avgpool_bwd(dy, (B, C, HW, 1))
    assert same_bits(wdx.permute(0, 2, 3, 1).reshape(B, HW, C), dx), "ops.global_avgpool_bwd differs from the direct call"


@pytest.mark.parametrize("Rr,n", [(1, 1), (5, 9), (7, 64), (6, 65), (7, 200)])
def test_softmax_rows(Rr, n):
    """inputs ~ N(0, 20^2): rows span more than +-60, so the max subtraction matters; the last row holds equal values; the backward
    pass takes the kernel's own y"""
    _lib, ops, lib = _api()
    g = _gen(80 + n)
    x_c, dy_c = torch.randn(Rr, n, generator=g) * 20, torch.randn(Rr, n, generator=g)
    x_c[Rr - 1] = 3.25
    x, dy = x_c.to(DEV), dy_c.to(DEV)
    G = Guards()
    y = G.out("y", Rr, n)
    _lib.call("vp_softmax_rows_fwd_f32", ops._p(x), ops._p(y), Rr, n, ops._stream())
    G.check()
    _tensor(y, R.softmax_rows_fwd(x_c), f"softmax_rows fwd {(Rr, n)}")
    rowsum = y.double().sum(dim=1).cpu()
    assert (rowsum - 1).abs().max().item() <= OP_RTOL, f"rows do not sum to 1: {rowsum.tolist()}"
    G = Guards()
    dx = G.out("dx", Rr, n)
    _lib.call("vp_softmax_rows_bwd_f32", ops._p(y), ops._p(dy), ops._p(dx), Rr, n, ops._stream())
    G.check()
    _tensor(dx, R.softmax_rows_bwd(y.cpu(), dy_c), f"softmax_rows bwd {(Rr, n)}")
    assert same_bits(ops.softmax_rows_fwd(x), y), "ops.softmax_rows_fwd differs from the direct call"
    assert same_bits(ops.softmax_rows_bwd(y, dy), dx), "ops.softmax_rows_bwd differs from the direct call"
