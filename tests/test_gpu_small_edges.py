"""The small kernels (csrc/elementwise.hip, optim.hip, score.hip, project.hip) at the shapes of tests/small_cases.py, on guarded
buffers: (a) every reduction returns the same bits on a second call, (b) vp_vae_loss_f32's recon has the bits of vp_bce_sum_f32's
result, (c) vp_adam_outer_f32 at K = 1 against vp_adam_f32 on the materialised gradient.

(c) relies on the forms of Adam's v that csrc/optim.h names and DESIGN.md section 25 lists per path.  vp_adam_f32, element i of n:
ADAM_V_FMA_SQUARE in the two-quad loop, ADAM_V_FMA_DECAY in a thread's last single quad, ADAM_V_TWO_PRODUCTS in the last n & 3
elements.  vp_adam_outer_f32, element (r, c): ADAM_V_FMA_SQUARE where r % 4 < 3 and c % 4 < 2, ADAM_V_TWO_PRODUCTS elsewhere.  m takes
one form everywhere.  So m has the same bits in every element, v and p where both kernels take ADAM_V_FMA_SQUARE; every element of
both is held to the fp64 step of tests/small_ref.py with the bounds of tests/test_gpu_flat_optim.py.  At K = 1 the contracted
gradient fma(a, b, 0) is the fp32 product a b, which is what vp_adam_f32 is given, with the same grad_scale."""
import pytest
import torch

from tests import small_cases as S
from tests import small_ref as R
from tests.guarded import Guards, same_bits
from tests.norm_cases import Lib
from tests.util import OP_RTOL, assert_close

pytestmark = pytest.mark.gpu

REDUCTIONS = [(fn, args) for fn, args, reduction in S.CASES if reduction]


@pytest.fixture(scope="module")
def lib():
    return Lib()


@pytest.mark.parametrize("fn,args", REDUCTIONS, ids=[f"{fn.__name__}{args}" for fn, args in REDUCTIONS])
def test_reduction_repeats_its_bits(lib, fn, args):
    first, second = fn(lib, *args), fn(lib, *args)
    assert first.keys() == second.keys()
    for k, a in first.items():
        b = second[k]
        assert (a is None) == (b is None), k
        if a is not None and a.dtype == torch.float32:
            assert same_bits(a, b), k
        elif a is not None:
            assert torch.equal(a, b), k


@pytest.mark.parametrize("n", [3, 1027, S.REDUCE_BIG])
def test_vae_loss_recon_is_bce_sum(lib, n):
    o = S.reduce_case(lib, n)
    assert same_bits(o["vae recon"], o["bce_sum"])


def adam_loop_mask(n):
    """elements of a flat array of n that adam_kernel updates in its two-quad loop (grid capped at 16384 blocks of 256 threads)"""
    n4 = n // 4
    stride = min(max((n4 + 1 + 255) // 256, 1), 16384) * 256
    q = torch.arange(n, dtype=torch.int64) // 4
    start, k = q % stride, q // stride
    quads = (n4 - start + stride - 1) // stride             # quads of the thread that owns this one
    return (q < n4) & (k < quads // 2 * 2)


@pytest.mark.parametrize("Rr,Cn", [(4, 4), (8, 1024), (12, 1028), (8, 4 * (524288 + 128))])
def test_adam_outer_one_product_against_adam(lib, Rr, Cn):
    from vae_play_amd import ops
    P, st = ops._pv, ops._stream()
    step, gs = 3, 0.25
    A, Bm, p0, m0, v0 = S.adam_outer_inputs(1, Rr, Cn)
    outer = S.adam_outer_case(lib, 1, Rr, Cn, step, gs)
    grad = A[0].cuda()[:, None] * Bm[0].cuda()[None, :]
    G = Guards()
    p, m, v = G.state("p", p0), G.state("m", m0), G.state("v", v0)
    n = Rr * Cn
    lib.call("vp_adam_f32", P(p), P(grad), P(m), P(v), n, S.LR, S.B1, S.B2, S.EPS, step, gs, st)
    G.check()
    rows, cols = torch.arange(Rr)[:, None], torch.arange(Cn)[None, :]
    both_square = ((rows % 4 < 3) & (cols % 4 < 2)) & adam_loop_mask(n).view(Rr, Cn)
    print(f"adam_outer ({Rr}, {Cn}): {int(both_square.sum())} of {n} elements take ADAM_V_FMA_SQUARE in both kernels")
    if n > 4 * 16384 * 256:
        assert both_square.any()
    assert same_bits(outer["m"], m)
    sel = both_square.cuda()
    assert same_bits(outer["v"][sel], v[sel]) and same_bits(outer["p"][sel], p[sel])
    f = [float(torch.tensor(x, dtype=torch.float32)) for x in (S.LR, S.B1, S.B2, S.EPS)]
    rp, rm, rv = R.adam_step(p0, A.double().t() @ Bm.double(), m0, v0, *f, step, gs)
    bound = 2e-7 * max(1.0, rp.abs().max().item())
    for name, got in (("outer", outer), ("adam", {"p": p, "m": m, "v": v})):
        d = (got["p"].cpu().double() - rp).abs().max().item()
        print(f"{name} ({Rr}, {Cn}): p max abs diff {d:.3e}, bound {bound:.3e}")
        assert d <= bound
        assert_close(got["m"].cpu(), rm, OP_RTOL, f"{name} m ({Rr}, {Cn})")
        assert_close(got["v"].cpu(), rv, OP_RTOL, f"{name} v ({Rr}, {Cn})")
