"""vp_adam_f32 and vp_rmsprop_f32 on guarded arenas against one fp64 step of tests/small_ref.py: two consecutive steps from non-zero
moments (the state step 1 writes is what step 2 reads), p, m, v (p, sq) compared after each step with the reference step applied
to the fp32 state the kernel started that step from.

Adam at n = 16,781,219 = 4 * (16384 * 256 + 1000) + 3 is the first size at which adam_kernel's two-quad loop with non-temporal
loads and stores runs (its grid is capped at 16384 blocks): 1000 threads take that loop, the others the single-quad path, three
elements the scalar tail.  RMSprop's grid is capped at 4096 blocks = 1,048,576 items: n = 2,101,155 takes a third trip.

Bounds: p to 2e-7 * max(1, max|p|) (the bound of test_gpu_parity.py::test_flat_optimizer_matches_torch); m, v, sq to OP_RTOL.  The
hyper-parameters are fp32-representable, so the kernel and the reference are asked for the same update."""
import pytest
import torch

from tests import small_ref as R
from tests.guarded import Guards, same_bits
from tests.guarded import api as _api
from tests.util import OP_RTOL, assert_close, record

pytestmark = pytest.mark.gpu
DEV = "cuda"


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32).item())


LR, B1, B2, EPS, ALPHA, GS = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(0.99), 0.25


def _p_close(got, ref, what):
    d = (got.double() - ref).abs().max().item()
    bound = 2e-7 * max(1.0, ref.abs().max().item())
    record(what + " (max abs diff / bound)", d / bound)
    print(f"{what}: max abs diff {d:.3e}, bound {bound:.3e}")
    assert d <= bound, f"{what}: {d:.3e} > {bound:.3e}"


def _draw(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.5 + 1e-3
    grads = [torch.randn(n, generator=g) * 2, torch.randn(n, generator=g) * 2]
    return p, m, v, grads


@pytest.mark.parametrize("n", [1, 7, 1027, 4 * (16384 * 256 + 1000) + 3])
def test_adam_two_steps(n):
    _lib, ops, lib = _api()
    p0, m0, v0, grads = _draw(n, 1500 + n % 97)
    G = Guards()
    p, m, v = G.state("p", p0), G.state("m", m0), G.state("v", v0)
    first_step = 3                       # not the first step of a run: both bias corrections differ from 1 and from each other
    for k, g_c in enumerate(grads):
        step = first_step + k
        g = g_c.to(DEV)
        _lib.call("vp_adam_f32", ops._p(p), ops._p(g), ops._p(m), ops._p(v), n, LR, B1, B2, EPS, step, GS, ops._stream())
        G.check()
        assert torch.equal(g.cpu(), g_c), "the gradient was modified"
        rp, rm, rv = R.adam_step(p0, g_c, m0, v0, LR, B1, B2, EPS, step, GS)
        p1, m1, v1 = p.cpu(), m.cpu(), v.cpu()
        _p_close(p1, rp, f"adam p n={n} step {k + 1}")
        e_m = assert_close(m1, rm, OP_RTOL, f"adam m n={n} step {k + 1}")
        e_v = assert_close(v1, rv, OP_RTOL, f"adam v n={n} step {k + 1}")
        print(f"adam n={n} step {k + 1}: m {e_m:.3e}, v {e_v:.3e}")
        if n < 100000:                   # the wrapper on a copy of the same state: same bits
            wp, wm, wv = p0.to(DEV), m0.to(DEV), v0.to(DEV)
            ops.adam_step(wp, g, wm, wv, LR, B1, B2, EPS, step, GS)
            assert same_bits(wp, p1) and same_bits(wm, m1) and same_bits(wv, v1), "ops.adam_step differs from the direct call"
        p0, m0, v0 = p1, m1, v1


@pytest.mark.parametrize("n", [1, 7, 1027, 2 * 1048576 + 4000 + 3])
def test_rmsprop_two_steps(n):
    _lib, ops, lib = _api()
    p0, _, sq0, grads = _draw(n, 1600 + n % 97)
    G = Guards()
    p, sq = G.state("p", p0), G.state("sq", sq0)
    for k, g_c in enumerate(grads):
        g = g_c.to(DEV)
        _lib.call("vp_rmsprop_f32", ops._p(p), ops._p(g), ops._p(sq), n, LR, ALPHA, EPS, GS, ops._stream())
        G.check()
        assert torch.equal(g.cpu(), g_c), "the gradient was modified"
        rp, rsq = R.rmsprop_step(p0, g_c, sq0, LR, ALPHA, EPS, GS)
        p1, sq1 = p.cpu(), sq.cpu()
        _p_close(p1, rp, f"rmsprop p n={n} step {k + 1}")
        e = assert_close(sq1, rsq, OP_RTOL, f"rmsprop sq n={n} step {k + 1}")
        print(f"rmsprop n={n} step {k + 1}: sq {e:.3e}")
        if n < 100000:
            wp, wsq = p0.to(DEV), sq0.to(DEV)
            ops.rmsprop_step(wp, g, wsq, LR, ALPHA, EPS, GS)
            assert same_bits(wp, p1) and same_bits(wsq, sq1), "ops.rmsprop_step differs from the direct call"
        p0, sq0 = p1, sq1
