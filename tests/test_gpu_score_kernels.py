"""The three scoring kernels of csrc/score.hip, each called through the C ABI on NaN-prefilled, sentinel-guarded outputs
(tests/guarded.py) and held to OP_RTOL against the fp64 restatements of tests/score_ref.py, evaluated on the same fp32 inputs.
What the bound is relative to: a sum of positive terms (the BCE of a row) and the values of the bound (one sign, magnitude 1e3 ..
1e5) to the reference value itself; lr, a SIGNED sum that cancels, to the sum of the absolute values of its terms (as vp_sum_f32 is
held in tests/test_gpu_small_losses.py).  Every reduction is run twice and must return the same bits.

Shapes of vp_bce_rows_f32: a single element; a row shorter than a wave with rows off the 16-byte grid (n = 7); exactly one pass of
a workgroup's 16-byte loads (1024) and one short of it (1023, every row start at another offset); n a multiple of 4 below one chunk
(3072); and 49 157 = 12 chunks of 4096 + 5, odd, so that the second stage, a short last chunk and the scalar head all run."""
from ctypes import c_void_p

import pytest
import torch

from tests import score_ref as R
from tests.guarded import Guards, same_bits
from tests.guarded import api as _api, gen as _gen, scalar_close as _scalar

pytestmark = pytest.mark.gpu
DEV = "cuda"

BCE_SHAPES = [(1, 1), (3, 7), (4, 1024), (5, 1023), (2, 3072), (3, 49157)]


def _bce_rows(lib, ops, _lib, p, t, rows, n):
    G = Guards()
    out = G.out("out", rows)
    ws, nb = G.ws("ws", lib.vp_bce_rows_workspace_bytes(rows, n))
    _lib.call("vp_bce_rows_f32", ops._p(p), ops._p(t), rows, n, ops._p(out), ops._p(ws), nb, ops._stream())
    G.check()
    return out.clone()


@pytest.mark.parametrize("rows,n", BCE_SHAPES)
def test_bce_rows(rows, n):
    _lib, ops, lib = _api()
    g = _gen(1000 + n % 97)
    p_c = 2e-6 + torch.rand(rows, n, generator=g) * (1.0 - 4e-6)
    t_c = torch.rand(rows, n, generator=g)
    assert 1e-6 < float(p_c.min()) and float(p_c.max()) < 1.0 - 1e-6
    p, t = p_c.to(DEV), t_c.to(DEV)
    runs = [_bce_rows(lib, ops, _lib, p, t, rows, n) for _ in range(2)]
    _scalar(runs[0], R.bce_rows(p_c, t_c), f"bce_rows {(rows, n)}")
    assert same_bits(runs[0], runs[1]), "two runs differ"
    assert same_bits(ops.bce_rows(p, t), runs[0]), "ops.bce_rows differs from the direct call"
    # the rows add up to the whole tensor's sum (vp_bce_sum_f32)
    _scalar(ops.bce_sum(p, t), runs[0].double().sum().cpu(), f"bce_rows {(rows, n)}: sum of rows against bce_sum")


@pytest.mark.parametrize("rows,n", [(3, 7), (2, 4101)])
def test_bce_rows_clamp(rows, n):
    """exact 0.0 and 1.0 in p against both targets: log is clamped at -100 before the product, so 0 x -inf never appears"""
    _lib, ops, lib = _api()
    g = _gen(1100 + n)
    p_c = 2e-6 + torch.rand(rows, n, generator=g) * (1.0 - 4e-6)
    t_c = torch.rand(rows, n, generator=g)
    for r in range(rows):       # at the head of the row, and in its last (scalar tail / last chunk) elements
        p_c[r, 0], p_c[r, 1], p_c[r, -2], p_c[r, -1] = 0.0, 0.0, 1.0, 1.0
        t_c[r, 0], t_c[r, 1], t_c[r, -2], t_c[r, -1] = 0.0, 1.0, 0.0, 1.0
    out = _bce_rows(lib, ops, _lib, p_c.to(DEV), t_c.to(DEV), rows, n)
    ref = R.bce_rows(p_c, t_c)
    assert (ref > 200.0).all()                      # (p = 0, t = 1) and (p = 1, t = 0) cost 100 each
    _scalar(out, ref, f"bce_rows clamp {(rows, n)}")


@pytest.mark.parametrize("off_p,off_t", [(1, 1), (3, 3), (0, 1)])
def test_bce_rows_off_the_16_byte_grid(off_p, off_t):
    """p and t that start off a 16-byte boundary: by the same amount (scalar head, then 16-byte loads), and by different amounts
    (element by element)"""
    _lib, ops, lib = _api()
    rows, n = 3, 4099
    g = _gen(1200 + 4 * off_p + off_t)
    p_c = 2e-6 + torch.rand(rows * n + 4, generator=g) * (1.0 - 4e-6)
    t_c = torch.rand(rows * n + 4, generator=g)
    p, t = p_c.to(DEV)[off_p:off_p + rows * n], t_c.to(DEV)[off_t:off_t + rows * n]
    assert p.data_ptr() % 16 == 4 * off_p and t.data_ptr() % 16 == 4 * off_t
    out = _bce_rows(lib, ops, _lib, p, t, rows, n)
    ref = R.bce_rows(p_c[off_p:off_p + rows * n].view(rows, n), t_c[off_t:off_t + rows * n].view(rows, n))
    _scalar(out, ref, f"bce_rows offsets {(off_p, off_t)}")


@pytest.mark.parametrize("B,Z", [(1, 1), (3, 16), (5, 130), (4, 512)])
def test_latent_iw_fwd(B, Z):
    _lib, ops, lib = _api()
    g = _gen(1300 + Z)
    mu_c, lv_c, eps_c = torch.randn(B, Z, generator=g), 0.5 * torch.randn(B, Z, generator=g) - 1.0, torch.randn(B, Z, generator=g)
    mu, lv, eps = mu_c.to(DEV), lv_c.to(DEV), eps_c.to(DEV)
    z0, kl0 = ops.latent_fwd(mu, lv, eps)
    runs = []
    for want_kl in (True, False, True):
        G = Guards()
        z, lr = G.out("z", B, Z), G.out("lr", B)
        kl = G.out("kl", B) if want_kl else None
        _lib.call("vp_latent_iw_fwd_f32", ops._p(mu), ops._p(lv), ops._p(eps), ops._p(z), ops._p(kl), ops._p(lr), B, Z, ops._stream())
        G.check()
        assert torch.equal(z, z0) and same_bits(z, z0), "z differs from vp_latent_fwd_f32"
        if want_kl:
            assert torch.equal(kl, kl0) and same_bits(kl, kl0), "kl differs from vp_latent_fwd_f32"
        runs.append(lr.clone())
    assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2]), "lr: runs differ"
    _, _, lr_ref, scale = R.latent_iw(mu_c, lv_c, eps_c)
    _scalar(runs[0], lr_ref, f"latent_iw lr {(B, Z)}", denom=scale)
    zo, klo, lro = ops.latent_iw_fwd(mu, lv, eps)
    assert same_bits(zo, z0) and same_bits(klo, kl0) and same_bits(lro, runs[0]), "ops.latent_iw_fwd differs from the direct call"
    # eps = 0: z = mu, and lr = 1/2 sum (logvar - mu^2)
    zero = torch.zeros_like(eps)
    z1, _, lr1 = ops.latent_iw_fwd(mu, lv, zero)
    assert torch.equal(z1, mu)
    want = 0.5 * (lv_c.double() - mu_c.double() ** 2).sum(1)
    _scalar(lr1, want, f"latent_iw lr at eps = 0 {(B, Z)}", denom=0.5 * (lv_c.double().abs() + mu_c.double() ** 2).sum(1))


def _iw(lib, ops, _lib, nbce, lr, want_logw=True):
    B, K = nbce.shape
    G = Guards()
    iwae = G.out("iwae", B)
    logw = G.out("logw", B, K) if want_logw else None
    _lib.call("vp_iw_bound_f32", ops._p(nbce), ops._p(lr), B, K, ops._p(logw), ops._p(iwae), ops._stream())
    G.check()
    return (logw.clone() if want_logw else None), iwae.clone()


@pytest.mark.parametrize("mag", (2e3, 1e5))
@pytest.mark.parametrize("B,K", [(1, 1), (3, 2), (2, 50), (2, 64), (2, 65)])
def test_iw_bound(B, K, mag):
    """K = 64 / 65: one full trip of the wave over the draws, and the first lane's second"""
    _lib, ops, lib = _api()
    g = _gen(1400 + K)
    nbce_c = mag + 30.0 * (2.0 * torch.rand(B, K, generator=g) - 1.0)
    lr_c = 5.0 * torch.randn(B, K, generator=g)
    nbce, lr = nbce_c.to(DEV), lr_c.to(DEV)
    logw, iwae = _iw(lib, ops, _lib, nbce, lr)
    logw_ref, iwae_ref = R.iw_bound(nbce_c, lr_c)
    assert float((logw_ref.max(1).values - logw_ref.min(1).values).max()) > (20.0 if K >= 50 else -1.0)     # exp underflows unshifted
    _scalar(logw, logw_ref, f"iw_bound logw {(B, K)} at {mag:g}")
    _scalar(iwae, iwae_ref, f"iw_bound iwae {(B, K)} at {mag:g}")
    assert same_bits(logw, lr - nbce)
    assert (iwae <= logw.max(1).values).all() and (iwae >= logw.min(1).values).all()
    again = _iw(lib, ops, _lib, nbce, lr, want_logw=False)[1]
    assert same_bits(iwae, again), "two runs (the second without logw) differ"
    lo, io = ops.iw_bound(nbce, lr)
    assert same_bits(lo, logw) and same_bits(io, iwae), "ops.iw_bound differs from the direct call"
    if K == 1:
        assert same_bits(iwae, logw[:, 0]), "K = 1 must return logw itself"
    # a row of equal values returns that value: the sum is K and log K - log K the round trip (allowed: 1 ulp)
    flat_n, flat_l = nbce[:, :1].expand(B, K).contiguous(), lr[:, :1].expand(B, K).contiguous()
    w, flat = _iw(lib, ops, _lib, flat_n, flat_l)
    ulp = torch.nextafter(w[:, 0].abs(), torch.full_like(w[:, 0], float("inf"))) - w[:, 0].abs()
    assert ((flat - w[:, 0]).abs() <= ulp).all(), (flat, w[:, 0])


def test_refusals():
    """null pointers, zero sizes and a short workspace return their codes and leave the outputs alone"""
    _lib, ops, lib = _api()
    st = ops._stream()
    P = lambda t: None if t is None else c_void_p(t.data_ptr())       # noqa: E731
    G = Guards()
    p, t = torch.rand(3, 5000, device=DEV), torch.rand(3, 5000, device=DEV)
    out = G.out("out", 3)
    need = lib.vp_bce_rows_workspace_bytes(3, 5000)
    assert need == 3 * 2 * 4 and lib.vp_bce_rows_workspace_bytes(0, 5) == 0 and lib.vp_bce_rows_workspace_bytes(5, 0) == 0
    ws, nb = G.ws("ws", need)
    ARG, WS = -1, -3
    assert lib.vp_bce_rows_f32(None, P(t), 3, 5000, P(out), P(ws), nb, st) == ARG
    assert lib.vp_bce_rows_f32(P(p), None, 3, 5000, P(out), P(ws), nb, st) == ARG
    assert lib.vp_bce_rows_f32(P(p), P(t), 3, 5000, None, P(ws), nb, st) == ARG
    assert lib.vp_bce_rows_f32(P(p), P(t), 3, 5000, P(out), None, nb, st) == ARG
    assert lib.vp_bce_rows_f32(P(p), P(t), 0, 5000, P(out), P(ws), nb, st) == ARG
    assert lib.vp_bce_rows_f32(P(p), P(t), 3, 0, P(out), P(ws), nb, st) == ARG
    assert b"vp_bce_rows_f32" in lib.vp_last_error()
    assert lib.vp_bce_rows_f32(P(p), P(t), 3, 5000, P(out), P(ws), nb - 4, st) == WS
    assert b"workspace" in lib.vp_last_error()
    mu = torch.randn(2, 8, device=DEV)
    z, lr, kl = G.out("z", 2, 8), G.out("lr", 2), G.out("kl", 2)
    for args in ((None, P(mu), P(mu), P(z), P(kl), P(lr), 2, 8), (P(mu), None, P(mu), P(z), P(kl), P(lr), 2, 8),
                 (P(mu), P(mu), None, P(z), P(kl), P(lr), 2, 8), (P(mu), P(mu), P(mu), None, P(kl), P(lr), 2, 8),
                 (P(mu), P(mu), P(mu), P(z), P(kl), None, 2, 8), (P(mu), P(mu), P(mu), P(z), P(kl), P(lr), 0, 8),
                 (P(mu), P(mu), P(mu), P(z), P(kl), P(lr), 2, 0)):
        assert lib.vp_latent_iw_fwd_f32(*args, st) == ARG
    iwae, logw = G.out("iwae", 2), G.out("logw", 2, 4)
    for args in ((None, P(mu), 2, 4, P(logw), P(iwae)), (P(mu), None, 2, 4, P(logw), P(iwae)), (P(mu), P(mu), 2, 4, P(logw), None),
                 (P(mu), P(mu), 0, 4, P(logw), P(iwae)), (P(mu), P(mu), 2, 0, P(logw), P(iwae))):
        assert lib.vp_iw_bound_f32(*args, st) == ARG
    torch.cuda.synchronize()
    for name, ib, buf, nan_ok in G.items:           # nothing was launched: every output still holds its NaN prefill
        assert torch.isnan(buf).all(), name
    # ... and the library stays usable
    assert lib.vp_bce_rows_f32(P(p), P(t), 3, 5000, P(out), P(ws), nb, st) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
