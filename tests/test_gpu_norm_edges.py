"""csrc/bn.hip at the edges of its grids, trips and kernels (tests/norm_cases.py), on guarded buffers with exact-size workspaces.
Every assertion is an identity that holds by construction, bit for bit: the entry points are different routes through the same
kernels, launched over the same grids, so no fixture and no tolerance is needed.  After every case the sentinels around each output
are intact and no output element is still NaN."""
import pytest
import torch

from tests import norm_cases as N
from tests.guarded import Guards, same_bits

pytestmark = pytest.mark.gpu

B1 = [(1, R, C) for R, C in N.BN_SHAPES if (1, R, C) not in N.BATCHED]
ids = lambda cases: ["x".join(map(str, c)) for c in cases]


def _act(*dims):
    """every activation is met somewhere on the case list"""
    return N.ACTS[sum(dims) % len(N.ACTS)]


def _same(a, b, what):
    assert a.dtype == b.dtype and (torch.equal(a, b) if a.dtype != torch.float32 else same_bits(a.reshape(-1), b.reshape(-1))), what


@pytest.mark.parametrize("B,R,C", N.BATCHED + B1, ids=ids(N.BATCHED + B1))
def test_instnorm_is_batchnorm_image_by_image(B, R, C):
    """(a) vp_instnorm_act_{fwd,bwd}_f32 on [B][R][C] against vp_bn_stats_f32 (no running statistics) + vp_bn_act_{fwd,bwd}_f32 with
    null gamma, beta, dgamma, dbeta and batch_stats = 1 on each image."""
    L, G, act = N.Lib(), Guards(), _act(B, R, C)
    x, dy = N.inputs(B, R, C)[:2]
    y, mean, rstd, _ = N.inorm_fwd(L, G, x, B, R, C, act)
    dx, _ = N.inorm_bwd(L, G, x, dy, mean, rstd, B, R, C, act)
    for b in range(B):
        m, r, _, _ = N.bn_stats(L, G, x[b], R, C)
        yb, _ = N.bn_fwd(L, G, "plain", x[b], m, r, None, None, R, C, act)
        dxb = N.bn_bwd(L, G, "plain", x[b], dy[b], m, r, None, None, R, C, act, affine_grads=False)[0]
        for got, ref, what in ((mean[b], m, "mean"), (rstd[b], r, "rstd"), (y[b], yb, "y"), (dx[b], dxb, "dx")):
            _same(got, ref, f"image {b}: {what}")
    G.check()


SPLITTABLE = [s for s in N.BN_SHAPES if s[1] % 4 == 0]


@pytest.mark.parametrize("R,C", SPLITTABLE, ids=ids(SPLITTABLE))
def test_entry_points_of_one_pass_agree(R, C):
    """(b) the four backward entry points (plain, split, split_fmt with format 0 and scale 1, split_fmt_sat) give the same dx, dgamma
    and dbeta, and planes that are ops.split_f32 of dx; the same for the three forward entry points."""
    from vae_play_amd import ops
    L, G, act = N.Lib(), Guards(), _act(R, C)
    x, dy, gamma, beta, _ = N.inputs(1, R, C)
    x, dy = x[0], dy[0]
    mean, rstd, _, _ = N.bn_stats(L, G, x, R, C)
    y0, _ = N.bn_fwd(L, G, "plain", x, mean, rstd, gamma, beta, R, C, act)
    want = ops.split_f32(y0)
    for kind in ("split", "fmt"):
        y, ys = N.bn_fwd(L, G, kind, x, mean, rstd, gamma, beta, R, C, act)
        _same(y, y0, f"forward {kind}: y")
        _same(ys, want, f"forward {kind}: planes")
    dx0, _, dg0, db0, _ = N.bn_bwd(L, G, "plain", x, dy, mean, rstd, gamma, beta, R, C, act)
    want = ops.split_f32(dx0)
    for kind in ("split", "fmt", "sat"):
        dx, ds, dg, db, sat = N.bn_bwd(L, G, kind, x, dy, mean, rstd, gamma, beta, R, C, act)
        for got, ref, what in ((dx, dx0, "dx"), (dg, dg0, "dgamma"), (db, db0, "dbeta"), (ds, want, "planes")):
            _same(got, ref, f"backward {kind}: {what}")
        assert sat is None or int(sat.item()) == 0, "the bf16 format cannot saturate"
    G.check()


@pytest.mark.parametrize("B,R,C", N.BATCHED, ids=ids(N.BATCHED))
def test_pair_blend_statistics_are_instnorm_over_the_stacked_channels(B, R, C):
    """(c) vp_pair_blend_fwd_f32 with norm = 1 returns the mean and rstd of vp_instnorm_act_fwd_f32 over the 2C stacked channels."""
    L, G, act = N.Lib(), Guards(), _act(B, R, C)
    u, _, _, _, label = N.inputs(B, R, 2 * C)
    _, mean, rstd, _ = N.pair_fwd(L, G, u, label, B, R, C, 1, act)
    _, m, r, _ = N.inorm_fwd(L, G, u, B, R, 2 * C, act)
    _same(mean, m, "mean")
    _same(rstd, r, "rstd")
    G.check()


@pytest.mark.parametrize("R,C", N.BN_SHAPES, ids=ids(N.BN_SHAPES))
def test_batchnorm_reductions_repeat(R, C):
    """(d) statistics, running statistics, dgamma, dbeta and dx come out the same on a second call."""
    L, G, act = N.Lib(), Guards(), _act(R, C)
    x, dy, gamma, beta, _ = N.inputs(1, R, C)
    x, dy = x[0], dy[0]
    first = N.bn_stats(L, G, x, R, C, running=True)
    for got, ref, what in zip(N.bn_stats(L, G, x, R, C, running=True), first, ("mean", "rstd", "running_mean", "running_var")):
        _same(got, ref, what)
    mean, rstd = first[:2]
    one, two = (N.bn_bwd(L, G, "plain", x, dy, mean, rstd, gamma, beta, R, C, act) for _ in range(2))
    for i, what in ((0, "dx"), (2, "dgamma"), (3, "dbeta")):
        _same(two[i], one[i], what)
    G.check()


@pytest.mark.parametrize("B,R,C", N.BATCHED, ids=ids(N.BATCHED))
def test_batched_reductions_repeat(B, R, C):
    """(d) InstanceNorm and the pair blend (norm = 1), forward and backward, come out the same on a second call."""
    L, G, act = N.Lib(), Guards(), _act(B, R, C)
    x, dy = N.inputs(B, R, C)[:2]
    y, mean, rstd, _ = N.inorm_fwd(L, G, x, B, R, C, act)
    for got, ref, what in zip(N.inorm_fwd(L, G, x, B, R, C, act)[:3], (y, mean, rstd), ("y", "mean", "rstd")):
        _same(got, ref, f"instnorm {what}")
    _same(N.inorm_bwd(L, G, x, dy, mean, rstd, B, R, C, act)[0], N.inorm_bwd(L, G, x, dy, mean, rstd, B, R, C, act)[0], "instnorm dx")
    u, _, _, _, label = N.inputs(B, R, 2 * C)
    y, mean, rstd, _ = N.pair_fwd(L, G, u, label, B, R, C, 1, act)
    for got, ref, what in zip(N.pair_fwd(L, G, u, label, B, R, C, 1, act)[:3], (y, mean, rstd), ("y", "mean", "rstd")):
        _same(got, ref, f"pair blend {what}")
    _same(N.pair_bwd(L, G, u, dy, label, mean, rstd, B, R, C, 1, act)[0], N.pair_bwd(L, G, u, dy, label, mean, rstd, B, R, C, 1, act)[0],
          "pair blend du")
    G.check()
