"""The three kernels of csrc/project.hip, each called through the C ABI on NaN-prefilled, sentinel-guarded outputs (tests/guarded.py)
against the fp64 restatements of tests/project_ref.py evaluated on the same fp32 inputs, and -- where the header promises bits --
against the fp32 expression or the sibling entry point that defines them.

vp_affine_relu_bwd_f32: (R, C) = (7, 8): less than one wave of quads; (130, 72): C no power of two, the scale index wraps inside a
thread's stride; (2 * 16 * 16, 64): a decoder block of the small plans; (3, 4096): the dense BatchNorm1d view (R = B); (5, 6): C % 4 != 0,
the element-by-element kernel.  vp_bce_masked_rows_bwd_f32: n = 1 and 5 (scalar head only), 768 (less than one pass of 16-byte
loads), 4096 / 4097 (one chunk exactly, one element into the second stage), 12291 = 3 chunks + 3, with every pointer 0..3 floats off
the 16-byte grid, together and apart.  vp_latent_adam_f32: Z below, at a fraction of and above one trip of the wave."""
from ctypes import c_void_p

import pytest
import torch

from tests import project_ref as R
from tests.guarded import Guards, same_bits
from tests.guarded import api as _api, gen as _gen, scalar_close as _scalar
from tests.util import OP_RTOL, assert_close, record

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARG, WS = -1, -3


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32).item())


# ---- vp_affine_relu_bwd_f32 ----------------------------------------------------------------------------------------------------
def _affine(lib, ops, _lib, dy, u, us, scale, R_, C, want_f32, want_split, inplace=False):
    G = Guards()
    n = R_ * C
    dx = (G.state("dx", dy.cpu()) if inplace else G.out("dx", n)) if want_f32 else None
    dxs = G.planes("dxs", n) if want_split else None
    src = dx if inplace else dy
    _lib.call("vp_affine_relu_bwd_f32", ops._p(src), ops._p(u), ops._pv(us), ops._p(scale), ops._p(dx), ops._pv(dxs), R_, C, ops._stream())
    G.check()
    return (dx.clone() if want_f32 else None), (dxs.clone() if want_split else None)


@pytest.mark.parametrize("R_,C", [(7, 8), (130, 72), (2 * 16 * 16, 64), (3, 4096), (5, 6)])
def test_affine_relu_bwd(R_, C):
    _lib, ops, lib = _api()
    g = _gen(2000 + R_ + C)
    n = R_ * C
    u_c = torch.relu(torch.randn(n, generator=g))                  # about half exact zeros, as a ReLU leaves them
    u_c[1], u_c[n // 2], u_c[n - 1] = -0.0, 0.0, -0.0              # negative zero is not > 0
    u_c[2], u_c[n - 2] = 1e-30, 3.0
    dy_c = torch.randn(n, generator=g)
    s_c = torch.randn(C, generator=g)                              # both signs: a masked element is a zero with the sign of dy * s
    dy, u, scale = dy_c.to(DEV), u_c.to(DEV), s_c.to(DEV)
    us = ops.split_f32(u)                                          # what a bf16x3 plan keeps of the block's output
    assert torch.equal(ops.unsplit(us) > 0, u > 0)
    want = (dy.view(R_, C) * scale * (u.view(R_, C) > 0)).view(n)  # the fp32 expression, left to right
    assert int((want == 0).sum()) > n // 4 and bool((torch.signbit(want) & (want == 0)).any())
    want_s = ops.split_f32(want)
    for name, uu, uus in (("fp32 u", u, None), ("split u", None, us)):
        dx, dxs = _affine(lib, ops, _lib, dy, uu, uus, scale, R_, C, True, True)
        assert same_bits(dx, want), f"{name}: fp32 dx differs from dy * scale * (u > 0)"
        assert torch.equal(dxs, want_s), f"{name}: split dx differs from vp_split_f32 of the fp32 result"
        only32, _ = _affine(lib, ops, _lib, dy, uu, uus, scale, R_, C, True, False)
        _, only16 = _affine(lib, ops, _lib, dy, uu, uus, scale, R_, C, False, True)
        assert same_bits(only32, want) and torch.equal(only16, want_s), f"{name}: one output alone differs"
        inpl, inpl_s = _affine(lib, ops, _lib, dy, uu, uus, scale, R_, C, True, True, inplace=True)
        assert same_bits(inpl, want) and torch.equal(inpl_s, want_s), f"{name}: dx = dy differs"
    e = assert_close(want, R.affine_relu_bwd(dy_c.view(R_, C), u_c.view(R_, C), s_c).view(n), OP_RTOL, f"affine_relu_bwd {(R_, C)}")
    print(f"affine_relu_bwd {(R_, C)}: {e:.3e}")
    o32, o16 = ops.affine_relu_bwd(dy, us, scale, want_f32=True, want_split=True)
    assert same_bits(o32, want) and torch.equal(o16, want_s), "ops.affine_relu_bwd differs from the direct call"


def test_affine_relu_bwd_off_the_16_byte_grid():
    """pointers that are not 16-byte aligned take the element-by-element kernel: the same bits"""
    _lib, ops, lib = _api()
    g = _gen(2100)
    R_, C = 9, 8
    n = R_ * C
    dy, u, scale = torch.randn(n + 1, generator=g).to(DEV)[1:], torch.relu(torch.randn(n + 1, generator=g)).to(DEV)[1:], torch.randn(C, generator=g).to(DEV)
    assert dy.data_ptr() % 16 == 4
    want = (dy.view(R_, C) * scale * (u.view(R_, C) > 0)).view(n)
    dx, dxs = _affine(lib, ops, _lib, dy, u, None, scale, R_, C, True, True)
    assert same_bits(dx, want) and torch.equal(dxs, ops.split_f32(want))


# ---- vp_bce_masked_rows_bwd_f32 ------------------------------------------------------------------------------------------------
OFFSETS = [(0, 0, 0, 0), (1, 1, 1, 1), (3, 3, 3, 3), (2, 2, 0, 1), (0, 1, 2, 3)]        # floats past a 16-byte boundary: p, t, mask, dlogit


def _off(t_c, off, count):
    """``count`` elements of the host tensor on the device, starting ``off`` floats past a 16-byte boundary"""
    buf = torch.empty(count + 4, device=DEV)
    buf[off:off + count].copy_(t_c.reshape(-1))
    v = buf[off:off + count]
    assert v.data_ptr() % 16 == 4 * off
    return v


def _bce_masked(lib, ops, _lib, p, t, mask, rows, n, off_d=0):
    G = Guards()
    out = G.out("out", rows)
    slack = G._new("dlogit", rows * n + 4, torch.float32, True)       # (the slack around an offset output keeps its NaN)
    slack.fill_(float("nan"))
    dl = slack[off_d:off_d + rows * n]
    ws, nb = G.ws("ws", lib.vp_bce_masked_rows_bwd_workspace_bytes(rows, n))
    _lib.call("vp_bce_masked_rows_bwd_f32", ops._p(p), ops._p(t), ops._p(mask), rows, n, ops._p(out), ops._p(dl), ops._p(ws), nb,
              ops._stream())
    G.check()
    assert not torch.isnan(dl).any(), "dlogit: elements never written"
    assert torch.isnan(slack[:off_d]).all() and torch.isnan(slack[off_d + rows * n:]).all(), "dlogit: written outside its rows"
    return out.clone(), dl.clone()


@pytest.mark.parametrize("n", [1, 5, 768, 4096, 4097, 12291])
def test_bce_masked_rows_bwd(n):
    _lib, ops, lib = _api()
    rows = 3
    g = _gen(2200 + n % 97)
    p_c = 2e-6 + torch.rand(rows, n, generator=g) * (1.0 - 4e-6)
    t_c = torch.rand(rows, n, generator=g)
    m_c = torch.rand(rows, n, generator=g) * (torch.rand(rows, n, generator=g) > 0.25)       # weights in [0, 1], a quarter exact zeros
    if n >= 5:          # the saturated pairs, at the head and in the last (scalar tail / last chunk) elements
        for r in range(rows):
            p_c[r, 0], t_c[r, 0], m_c[r, 0] = 0.0, 1.0, 0.5
            p_c[r, -1], t_c[r, -1], m_c[r, -1] = 1.0, 0.0, 1.0
    ref, dl_ref = R.bce_masked_rows(p_c, t_c, m_c)
    ref1, _ = R.bce_masked_rows(p_c, t_c, None)
    for op, ot, om, od in OFFSETS:
        p, t, m = _off(p_c, op, rows * n), _off(t_c, ot, rows * n), _off(m_c, om, rows * n)
        what = f"bce_masked_rows {(rows, n)} offsets {(op, ot, om, od)}"
        out, dl = _bce_masked(lib, ops, _lib, p, t, m, rows, n, od)
        _scalar(out, ref, what)
        assert same_bits(dl, m * (p - t)), f"{what}: dlogit differs from fp32 mask * (p - t)"
        assert_close(dl, dl_ref.reshape(-1), OP_RTOL, what + " dlogit")
        again = _bce_masked(lib, ops, _lib, p, t, m, rows, n, od)
        assert same_bits(out, again[0]) and same_bits(dl, again[1]), f"{what}: two runs differ"
        # no mask: all ones, and the bits of vp_bce_rows_f32 on the same pointers
        out1, dl1 = _bce_masked(lib, ops, _lib, p, t, None, rows, n, od)
        _scalar(out1, ref1, what + " (no mask)")
        assert same_bits(dl1, p - t), f"{what}: dlogit without a mask differs from fp32 p - t"
        G = Guards()
        plain = G.out("plain", rows)
        ws, nb = G.ws("ws", lib.vp_bce_rows_workspace_bytes(rows, n))
        _lib.call("vp_bce_rows_f32", ops._p(p), ops._p(t), rows, n, ops._p(plain), ops._p(ws), nb, ops._stream())
        G.check()
        assert same_bits(out1, plain), f"{what}: mask = NULL differs from vp_bce_rows_f32"
        ones = torch.ones_like(p)
        assert same_bits(_bce_masked(lib, ops, _lib, p, t, ones, rows, n, od)[0], out1), f"{what}: a mask of ones differs from no mask"
    o, d = ops.bce_masked_rows_bwd(p_c.to(DEV), t_c.to(DEV), m_c.to(DEV))
    _scalar(o, ref, f"ops.bce_masked_rows_bwd {(rows, n)}")
    assert same_bits(d, m_c.to(DEV) * (p_c.to(DEV) - t_c.to(DEV)))


@pytest.mark.parametrize("n", [5, 4101])
def test_bce_masked_rows_bwd_saturated_pairs_cost_100_times_mask(n):
    """rows of nothing but (p = 0, t = 1) and (p = 1, t = 0): the logarithm is clamped at -100 before the product, each pair costs
    100 x its mask, exactly (every term and every partial sum is a multiple of 12.5 far below 2^24)"""
    _lib, ops, lib = _api()
    rows = 2
    i = torch.arange(rows * n).view(rows, n)
    p_c = (i % 2).float()
    t_c = 1.0 - p_c
    m_c = ((i * 7) % 9).float() / 8.0                      # 0, 1/8 .. 1
    out, dl = _bce_masked(lib, ops, _lib, p_c.to(DEV), t_c.to(DEV), m_c.to(DEV), rows, n)
    assert torch.equal(out.cpu(), 100.0 * m_c.sum(1)), (out, 100.0 * m_c.sum(1))
    assert torch.equal(dl.cpu().view(rows, n), m_c * (p_c - t_c))
    out1, _ = _bce_masked(lib, ops, _lib, p_c.to(DEV), t_c.to(DEV), None, rows, n)
    assert torch.equal(out1.cpu(), torch.full((rows,), 100.0 * n))


# ---- vp_latent_adam_f32 --------------------------------------------------------------------------------------------------------
LR, B1, B2, EPS = f32(0.05), f32(0.9), f32(0.999), f32(1e-8)


def _p_close(got, ref, what):
    """the bound tests/test_gpu_flat_optim.py holds vp_adam_f32's parameters to"""
    d = (got.double() - ref).abs().max().item()
    bound = 2e-7 * max(1.0, ref.abs().max().item())
    record(what + " (max abs diff / bound)", d / bound)
    print(f"{what}: max abs diff {d:.3e}, bound {bound:.3e}")
    assert d <= bound, f"{what}: {d:.3e} > {bound:.3e}"


@pytest.mark.parametrize("pw", [0.0, f32(0.75)])
@pytest.mark.parametrize("rows,Z", [(1, 8), (3, 16), (5, 130)])
def test_latent_adam_three_steps(rows, Z, pw):
    _lib, ops, lib = _api()
    g = _gen(2300 + Z)
    z0, m0, v0 = torch.randn(rows, Z, generator=g), torch.randn(rows, Z, generator=g) * 0.1, torch.rand(rows, Z, generator=g) * 0.5 + 1e-3
    grads = [torch.randn(rows, Z, generator=g) * 2 for _ in range(3)]
    G = Guards()
    z, m, v = G.state("z", z0), G.state("m", m0), G.state("v", v0)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k, g_c in enumerate(grads):
        step = k + 1
        gd = g_c.to(DEV)
        prior = G.out(f"prior{k}", rows)
        _lib.call("vp_latent_adam_f32", ops._p(z), ops._p(gd), ops._p(m), ops._p(v), c_void_p(count.data_ptr()), rows, Z, LR, B1, B2, EPS,
                  pw, ops._p(prior), ops._stream())
        G.check()
        assert int(count.item()) == step, "the device counter was not advanced by one"
        assert torch.equal(gd.cpu(), g_c), "the gradient was modified"
        rz, rm, rv, rprior = R.latent_adam(z0, g_c, m0, v0, step, LR, B1, B2, EPS, pw)
        z1, m1, v1 = z.cpu(), m.cpu(), v.cpu()
        what = f"latent_adam {(rows, Z)} pw={pw:g} step {step}"
        _p_close(z1, rz, what + " z")
        e_m, e_v = assert_close(m1, rm, OP_RTOL, what + " m"), assert_close(v1, rv, OP_RTOL, what + " v")
        print(f"{what}: m {e_m:.3e}, v {e_v:.3e}")
        if pw:
            _scalar(prior, rprior, what + " prior")
        else:
            assert torch.equal(prior.cpu(), torch.zeros(rows))
        # the same state through the wrapper (its own counter, at the same step): the same bits, and the prior alone too
        wz, wm, wv = z0.to(DEV), m0.to(DEV), v0.to(DEV)
        wcount = torch.full((1,), k, dtype=torch.int32, device=DEV)
        wprior = ops.latent_adam_step(wz, gd, wm, wv, wcount, LR, B1, B2, EPS, pw, want_prior=True)
        assert same_bits(wz, z1) and same_bits(wm, m1) and same_bits(wv, v1) and same_bits(wprior, prior), "ops.latent_adam_step differs"
        assert same_bits(ops.latent_prior(z0.to(DEV), pw), prior), "the prior alone differs from the update's"
        if pw == 0.0:       # vp_adam_f32 at the same (host) step on the same inputs: the same bits
            az, am, av = z0.to(DEV), m0.to(DEV), v0.to(DEV)
            _lib.call("vp_adam_f32", ops._p(az), ops._p(gd), ops._p(am), ops._p(av), rows * Z, LR, B1, B2, EPS, step, 1.0, ops._stream())
            assert same_bits(az, z1) and same_bits(am, m1) and same_bits(av, v1), f"{what}: differs from vp_adam_f32"
        z0, m0, v0 = z1, m1, v1
    assert int(count.item()) == 3


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """null pointers, non-positive sizes and a short workspace return their codes and leave the outputs alone"""
    _lib, ops, lib = _api()
    st = ops._stream()
    P = lambda t: None if t is None else c_void_p(t.data_ptr())       # noqa: E731
    G = Guards()
    # vp_affine_relu_bwd_f32
    dy, u, scale = torch.randn(4 * 8, device=DEV), torch.rand(4 * 8, device=DEV), torch.randn(8, device=DEV)
    us = ops.split_f32(u)
    dx, dxs = G.out("dx", 4 * 8), G.planes("dxs", 4 * 8)
    for args in ((None, P(u), None, P(scale), P(dx), P(dxs), 4, 8), (P(dy), P(u), None, None, P(dx), P(dxs), 4, 8),
                 (P(dy), None, None, P(scale), P(dx), P(dxs), 4, 8),              # no output of the block
                 (P(dy), P(u), P(us), P(scale), P(dx), P(dxs), 4, 8),             # both forms of it
                 (P(dy), P(u), None, P(scale), None, None, 4, 8),                 # nothing to write
                 (P(dy), P(u), None, P(scale), P(dx), P(dxs), 0, 8), (P(dy), P(u), None, P(scale), P(dx), P(dxs), 4, 0),
                 (P(dy), P(u), None, P(scale), P(dx), P(dxs), 4, -8)):
        assert lib.vp_affine_relu_bwd_f32(*args, st) == ARG, args
    assert b"vp_affine_relu_bwd_f32" in lib.vp_last_error()
    # vp_bce_masked_rows_bwd_f32
    p, t, mk = torch.rand(3, 5000, device=DEV), torch.rand(3, 5000, device=DEV), torch.rand(3, 5000, device=DEV)
    out, dl = G.out("out", 3), G.out("dl", 3 * 5000)
    need = lib.vp_bce_masked_rows_bwd_workspace_bytes(3, 5000)
    assert need == 3 * 2 * 4 and lib.vp_bce_masked_rows_bwd_workspace_bytes(0, 5) == 0 and lib.vp_bce_masked_rows_bwd_workspace_bytes(5, 0) == 0
    ws, nb = G.ws("ws", need)
    for args in ((None, P(t), P(mk), 3, 5000, P(out), P(dl), P(ws), nb), (P(p), None, P(mk), 3, 5000, P(out), P(dl), P(ws), nb),
                 (P(p), P(t), P(mk), 3, 5000, None, P(dl), P(ws), nb), (P(p), P(t), P(mk), 3, 5000, P(out), None, P(ws), nb),
                 (P(p), P(t), P(mk), 3, 5000, P(out), P(dl), None, nb), (P(p), P(t), P(mk), 0, 5000, P(out), P(dl), P(ws), nb),
                 (P(p), P(t), P(mk), 3, 0, P(out), P(dl), P(ws), nb), (P(p), P(t), P(mk), -3, 5000, P(out), P(dl), P(ws), nb)):
        assert lib.vp_bce_masked_rows_bwd_f32(*args, st) == ARG, args
    assert b"vp_bce_masked_rows_bwd_f32" in lib.vp_last_error()
    assert lib.vp_bce_masked_rows_bwd_f32(P(p), P(t), P(mk), 3, 5000, P(out), P(dl), P(ws), nb - 4, st) == WS
    assert b"workspace" in lib.vp_last_error()
    # vp_latent_adam_f32
    z0 = torch.randn(2, 8)
    z, m, v = G.state("z", z0), G.state("m", z0), G.state("v", z0.abs())
    gr, count, prior = torch.randn(2, 8, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), G.out("prior", 2)
    hyp = (LR, B1, B2, EPS, 1.0)
    for args in ((None, P(gr), P(m), P(v), P(count), 2, 8, *hyp, P(prior)), (P(z), None, P(m), P(v), P(count), 2, 8, *hyp, P(prior)),
                 (P(z), P(gr), None, P(v), P(count), 2, 8, *hyp, P(prior)), (P(z), P(gr), P(m), None, P(count), 2, 8, *hyp, P(prior)),
                 (P(z), P(gr), P(m), P(v), None, 2, 8, *hyp, P(prior)), (P(z), P(gr), P(m), P(v), P(count), 0, 8, *hyp, P(prior)),
                 (P(z), P(gr), P(m), P(v), P(count), 2, 0, *hyp, P(prior)), (P(z), P(gr), P(m), P(v), P(count), 2, -8, *hyp, P(prior)),
                 (P(z), None, None, None, None, 2, 8, *hyp, None),                 # the prior alone, with nowhere to put it
                 (P(z), P(gr), P(m), P(v), P(count), 2, 8, LR, 1.0, B2, EPS, 1.0, P(prior))):      # beta1 = 1
        assert lib.vp_latent_adam_f32(*args, st) == ARG, args
    assert b"vp_latent_adam_f32" in lib.vp_last_error()
    torch.cuda.synchronize()
    for name, ib, buf, nan_ok in G.items:           # nothing was launched: outputs still hold their NaN prefill, state its values
        if name in ("z", "m", "v"):
            assert torch.equal(buf.cpu().view(2, 8), z0 if name != "v" else z0.abs()), name
        else:
            assert (torch.isnan(buf).all() if buf.dtype == torch.float32 else (buf == 0x7FC0).all()), name
    assert int(count.item()) == 0
    # ... and the library stays usable
    assert lib.vp_bce_masked_rows_bwd_f32(P(p), P(t), P(mk), 3, 5000, P(out), P(dl), P(ws), nb, st) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and not torch.isnan(dl).any()
