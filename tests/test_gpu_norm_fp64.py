"""csrc/bn.hip against a float64 reference (tests/norm_ref.py) at the edges of its grids, trips and kernels (tests/norm_cases.py), on
guarded buffers with exact-size workspaces: BatchNorm statistics, running statistics, forward and backward; the one-launch small
BatchNorm; the eval-mode and null-affine backward through every entry point; InstanceNorm, also into a channel slice of a wider
buffer; the backward's fp16-format planes with a scale and the saturation flag.

Every output must lie within K[output] x S of the reference, S being the first-order fp32 error of a correct implementation
(norm_ref.scales) and K a constant per output kind fixed on the CPU (tests/test_norm_ref_cpu.py).  For ReLU and leaky ReLU the
backward reference takes the mask of the GPU's own forward output -- forward and backward round bn_pre identically -- and that mask
must be the fp64 one wherever |u| > K[y] S_y, so a wrong mask is caught either there or by dx."""
import pytest
import torch

from tests import norm_cases as N
from tests import norm_ref as NR
from tests.guarded import Guards, same_bits
from tests.util import record

pytestmark = pytest.mark.gpu

ids = lambda cases: ["x".join(map(str, c)) for c in cases]
WORST = {}        # output kind -> (worst ratio of this session, where)


def _verify(c, x, dy, kw, got, tag=""):
    """got: the GPU's outputs of case c (None: not asked for) against reference(x, dy, **kw), in units of K S"""
    masked = c["act"] in NR.MASKED
    ref = NR.reference(x, dy, mask=(got["y"].cpu() > 0) if masked else None, **kw)
    S = NR.scales(ref)
    what = NR.case_id(c) + tag
    r = NR.ratios(got, ref, S)
    for k, v in r.items():
        record(f"{what} {k} / S", v)
        if v > WORST.get(k, (0.0, ""))[0]:
            WORST[k] = (v, what)
    print(what, {k: round(v, 3) for k, v in r.items()})
    if masked:
        n = NR.mask_disagreements(got["y"], ref, S)
        assert n == 0, f"{what}: the forward's activation mask differs from the fp64 mask at {n} elements with |u| > K S"
    over = {k: v for k, v in r.items() if not v <= NR.K[k]}
    assert not over, f"{what}: beyond K x S: {over} (K = {({k: NR.K[k] for k in over})})"


def _report():
    print("worst ratio per output so far:", {k: (round(v, 3), w) for k, (v, w) in sorted(WORST.items())})


def _bn_inputs(R, C):
    dev = N.inputs(1, R, C)
    x, dy, gamma, beta = dev[0][0], dev[1][0], dev[2], dev[3]
    return (x, dy, gamma, beta), tuple(t.cpu() for t in (x, dy, gamma, beta))


@pytest.mark.parametrize("R,C", N.BN_SHAPES, ids=ids(N.BN_SHAPES))
def test_batchnorm_against_fp64(R, C):
    """(a) vp_bn_stats_f32 with running statistics, vp_bn_act_fwd_f32, vp_bn_act_bwd_f32 for every activation; at the SMALL shapes
    also vp_bn_small_fwd_f32 / vp_bn_small_bwd_f32, held to the reference on their own."""
    L = N.Lib()
    (x, dy, gamma, beta), (xc, dyc, gc, bc) = _bn_inputs(R, C)
    for act in N.ACTS:
        c = dict(kind="bn", B=1, R=R, C=C, act=act)
        kw = NR.case_args(c, xc, dyc, gc, bc)
        G = Guards()
        mean, rstd, rm, rv = N.bn_stats(L, G, x, R, C, running=True, momentum=NR.MOMENTUM)
        y, _ = N.bn_fwd(L, G, "plain", x, mean, rstd, gamma, beta, R, C, act)
        dx, _, dg, db, _ = N.bn_bwd(L, G, "plain", x, dy, mean, rstd, gamma, beta, R, C, act)
        G.check()
        _verify(c, xc, dyc, kw, dict(mean=mean, rstd=rstd, running_mean=rm, running_var=rv, y=y, dx=dx, dgamma=dg, dbeta=db))
        if (R, C) in N.SMALL:
            G = Guards()
            y, mean, rstd, rm, rv = N.bn_small_fwd(L, G, x, gamma, beta, R, C, act, running=True, momentum=NR.MOMENTUM)
            dx, dg, db = N.bn_small_bwd(L, G, x, dy, mean, rstd, gamma, beta, R, C, act)
            G.check()
            _verify(c, xc, dyc, kw, dict(mean=mean, rstd=rstd, running_mean=rm, running_var=rv, y=y, dx=dx, dgamma=dg, dbeta=db), " small")
    _report()


@pytest.mark.parametrize("variant,batch_stats", NR.BWD_VARIANTS, ids=[f"{v}-bs{b}" for v, b in NR.BWD_VARIANTS])
@pytest.mark.parametrize("R,C", NR.BWD_SHAPES, ids=ids(NR.BWD_SHAPES))
def test_backward_variants_against_fp64(R, C, variant, batch_stats):
    """(b) batch_stats = 0 with given mean and rstd; gamma, beta null with dgamma, dbeta asked for; gamma, beta given with dgamma,
    dbeta null -- through plain, split, fmt and sat where C % 4 == 0, through vp_bn_act_bwd_f32 alone where the planes are refused."""
    L = N.Lib()
    (x, dy, gamma, beta), (xc, dyc, gc, bc) = _bn_inputs(R, C)
    if variant == "null_affine":
        gamma = beta = None
    for act in N.ACTS:
        c = dict(kind="bwd", B=1, R=R, C=C, act=act, variant=variant, batch_stats=batch_stats)
        kw = NR.case_args(c, xc, dyc, gc, bc)
        G = Guards()
        if batch_stats:
            mean, rstd, _, _ = N.bn_stats(L, G, x, R, C)
        else:
            mean, rstd = (G.state(n, t) for n, t in zip(("mean", "rstd"), (kw["mean"], kw["rstd"])))
        y, _ = N.bn_fwd(L, G, "plain", x, mean, rstd, gamma, beta, R, C, act)
        for kind in ("plain", "split", "fmt", "sat") if C % 4 == 0 else ("plain",):
            dx, _, dg, db, sat = N.bn_bwd(L, G, kind, x, dy, mean, rstd, gamma, beta, R, C, act, batch_stats=batch_stats,
                                          affine_grads=variant != "no_affine_grads")
            G.check()
            assert sat is None or int(sat.item()) == 0, "the bf16 format cannot saturate"
            got = dict(y=y, dx=dx, dgamma=dg, dbeta=db)
            if batch_stats:
                got.update(mean=mean, rstd=rstd)
            _verify(c, xc, dyc, kw, got, " " + kind)
    _report()


INORM = [(B, R, C, 0.0) for B, R, C in N.BATCHED] + [(B, R, C, N.OFFSET) for B, R, C in N.OFFSET_BATCHED]


@pytest.mark.parametrize("B,R,C,offset", INORM, ids=[f"{B}x{R}x{C}" + ("-offset" if o else "") for B, R, C, o in INORM])
def test_instnorm_against_fp64(B, R, C, offset):
    """(c) vp_instnorm_act_fwd_f32 and vp_instnorm_act_bwd_f32: per-image mean, rstd, y and dx.  With the per-image offset of 300 a
    statistic, pivot or slab of another image is 1e-2 off in rstd where the right one is within 4e-7; every activation there."""
    L = N.Lib()
    x, dy = N.inputs(B, R, C, offset=offset)[:2]
    xc, dyc = x.cpu(), dy.cpu()
    for act in N.ACTS if offset else (NR.inorm_act(B, R, C),):
        c = dict(kind="inorm", B=B, R=R, C=C, act=act, offset=offset)
        G = Guards()
        y, mean, rstd, _ = N.inorm_fwd(L, G, x, B, R, C, act)
        dx, _ = N.inorm_bwd(L, G, x, dy, mean, rstd, B, R, C, act)
        G.check()
        _verify(c, xc, dyc, NR.case_args(c, xc, dyc, None, None), dict(mean=mean, rstd=rstd, y=y, dx=dx))
    _report()


@pytest.mark.parametrize("B,R,C", [(3, 65, 68), (1, 200, 8)], ids=ids([(3, 65, 68), (1, 200, 8)]))
def test_instnorm_into_a_channel_slice(B, R, C):
    """(c) vp_instnorm_act_fwd_ld_f32 with ldy = 2C at column offset C of a NaN-filled [B][R][2C] buffer: the slice is the dense call
    bit for bit, columns [0, C) are still NaN"""
    L, G, act = N.Lib(), Guards(), NR.inorm_act(B, R, C)
    x = N.inputs(B, R, C)[0]
    y, mean, rstd, _ = N.inorm_fwd(L, G, x, B, R, C, act)
    wide, m, r = N.inorm_fwd_ld(L, G, x, B, R, C, act, 2 * C, C)
    G.check()
    assert same_bits(wide[..., C:].contiguous(), y), "the slice differs from the dense call"
    assert bool(torch.isnan(wide[..., :C]).all()), "columns outside the slice were written"
    assert same_bits(m, mean) and same_bits(r, rstd), "statistics differ from the dense call"


def _f16_planes(dx, scale):
    """csrc/split.h split_f16 of dx * scale on the host -> int16 (2, n): clamp at +-65504, hi = half(x), lo = half(x - float(hi))"""
    xs = (dx.detach().cpu().reshape(-1) * torch.tensor(scale, dtype=torch.float32)).clamp(-65504.0, 65504.0)
    hi = xs.to(torch.float16)
    lo = (xs - hi.float()).to(torch.float16)
    return torch.stack([hi.view(torch.int16), lo.view(torch.int16)])


@pytest.mark.parametrize("R,C", NR.FMT_SHAPES, ids=ids(NR.FMT_SHAPES))
def test_backward_f16_planes_scale_and_saturation(R, C):
    """(d) vp_bn_act_bwd_split_fmt_sat_f32 with fmt = 1: at scale 2^10 the flag stays 0, at a scale that puts max |dx| just beyond
    65504 it is 1; the planes are split.h's of the GPU's own dx either way, and dx, dgamma, dbeta are the plain call's bits"""
    L = N.Lib()
    (x, dy, gamma, beta), _ = _bn_inputs(R, C)
    for act in N.ACTS:
        G = Guards()
        mean, rstd, _, _ = N.bn_stats(L, G, x, R, C)
        dx0, _, dg0, db0, _ = N.bn_bwd(L, G, "plain", x, dy, mean, rstd, gamma, beta, R, C, act)
        top = dx0.abs().max().cpu()
        over = float(torch.tensor(65504.0) / top * torch.tensor(1.0 + 2.0 ** -10))        # fp32 throughout, as the kernel multiplies
        assert float(top * torch.tensor(over)) > 65504.0 and float(top) * 1024.0 < 65504.0
        for scale, flag in ((1024.0, 0), (over, 1)):
            dx, ds, dg, db, sat = N.bn_bwd(L, G, "sat", x, dy, mean, rstd, gamma, beta, R, C, act, fmt=1, scale=scale)
            G.check()
            tag = f"act {act} scale {scale!r}"
            assert int(sat.item()) == flag, f"{tag}: saturation flag {int(sat.item())}, expected {flag}"
            for a, b, what in ((dx, dx0, "dx"), (dg, dg0, "dgamma"), (db, db0, "dbeta")):
                assert same_bits(a, b), f"{tag}: {what} differs from the plain call"
            want = _f16_planes(dx, scale)
            bad = int((ds.cpu() != want).sum())
            assert bad == 0, f"{tag}: {bad} of {want.numel()} plane elements differ from split_f16(dx * scale)"
            assert flag == 0 or int((want[0].view(torch.float16).float().abs() == 65504.0).sum()) >= 1, "nothing was clamped"
