"""tests/norm_ref.py on the CPU: the float64 reference against torch's autograd, the fp32 restatement of csrc/bn.hip against the
reference within K / 4 in units of the error scales (which is where K comes from), the activation masks of a correct fp32
implementation, and planted faults that the bound K must catch."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as NR

ACTS = NR.N.ACTS
SLOPE, EPS, MOM = 0.2, 1e-5, 0.1


def _torch_act(u, act):
    return {NR.ACT_NONE: lambda t: t, NR.ACT_RELU: F.relu, NR.ACT_LRELU: lambda t: F.leaky_relu(t, SLOPE), NR.ACT_TANH: torch.tanh,
            NR.ACT_SIGMOID: torch.sigmoid}[act](u)


def _close(got, want, what):
    err = (got - want).abs().max().item() / max(want.abs().max().item(), 1.0)       # inputs are O(1); at R = 1 y and dx are 0 and torch is 1e-14 off
    assert err <= 1e-12, f"{what}: {err:.3e}"


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "null-affine"])
@pytest.mark.parametrize("batch_stats", [1, 0])
@pytest.mark.parametrize("R,C", [(1, 4), (7, 8), (70, 3), (65, 68)])
def test_reference_is_torch_batch_norm_autograd(R, C, batch_stats, affine):
    g = torch.Generator().manual_seed(R * 131 + C)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x0, dy = rnd(R, C) * 1.5 + rnd(1, C) * 3, rnd(R, C)
    gamma, beta = (rnd(C) * 0.3 + 1, rnd(C) * 0.3) if affine else (None, None)
    mean, rstd = (None, None) if batch_stats else (rnd(C), torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
    rm0, rv0 = rnd(C), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    for act in ACTS:
        x = x0.clone().requires_grad_(True)
        w, b = (gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)) if affine else (None, None)
        rm, rv = rm0.clone(), rv0.clone()
        if batch_stats:     # F.batch_norm refuses one value per channel in training mode; this is the function it calls
            track = R > 1
            n = torch.batch_norm(x, w, b, rm if track else None, rv if track else None, True, MOM, EPS, False)
        else:
            n = F.batch_norm(x, mean, 1 / rstd ** 2 - EPS, w, b, False, MOM, EPS)
        y = _torch_act(n, act)
        (y * dy).sum().backward()
        ref = NR.reference(x0, dy, gamma, beta, act, SLOPE, EPS, MOM, batch_stats, mean=mean, rstd=rstd, rm=rm0, rv=rv0)
        tag = f"act {act}"
        _close(ref["y"], y.detach(), f"{tag}: y")
        _close(ref["dx"], x.grad, f"{tag}: dx")
        if affine:
            _close(ref["dgamma"], w.grad, f"{tag}: dgamma")
            _close(ref["dbeta"], b.grad, f"{tag}: dbeta")
        if batch_stats:
            _close(ref["mean"], x0.mean(0), f"{tag}: mean")
            _close(ref["rstd"], 1 / torch.sqrt(x0.var(0, unbiased=False) + EPS), f"{tag}: rstd")
        if batch_stats and R > 1:
            _close(ref["running_mean"], rm, f"{tag}: running_mean")
            _close(ref["running_var"], rv, f"{tag}: running_var")
        if R == 1:          # bn_finalize leaves the variance of one row biased: 0
            _close(ref["running_mean"], (1 - MOM) * rm0 + MOM * x0[0], f"{tag}: running_mean at R = 1")
            _close(ref["running_var"], (1 - MOM) * rv0, f"{tag}: running_var at R = 1")


def test_reference_is_torch_instance_norm_autograd():
    B, R, C = 3, 17, 6
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(B, R, C, generator=g, dtype=torch.float64) * 1.5 + torch.randn(B, 1, C, generator=g, dtype=torch.float64) * 3
    dy = torch.randn(B, R, C, generator=g, dtype=torch.float64)
    for act in ACTS:
        x = x0.clone().requires_grad_(True)
        y = _torch_act(F.instance_norm(x.transpose(1, 2), eps=EPS).transpose(1, 2), act)
        (y * dy).sum().backward()
        ref = NR.reference(x0, dy, None, None, act, SLOPE, EPS, 0.0, 1)
        _close(ref["y"], y.detach(), f"act {act}: y")
        _close(ref["dx"], x.grad, f"act {act}: dx")
        _close(ref["mean"], x0.mean(1), f"act {act}: mean")
        _close(ref["rstd"], 1 / torch.sqrt(x0.var(1, unbiased=False) + EPS), f"act {act}: rstd")


def test_reference_takes_a_given_mask():
    """with mask the ReLU and leaky-ReLU derivative follows the mask, not the sign of u"""
    x, dy = torch.randn(9, 4, dtype=torch.float64), torch.ones(9, 4, dtype=torch.float64)
    for act, low in ((NR.ACT_RELU, 0.0), (NR.ACT_LRELU, SLOPE)):
        ref = NR.reference(x, dy, None, None, act, SLOPE, EPS, MOM, 0, mask=torch.zeros(9, 4, dtype=torch.bool))
        assert torch.equal(ref["g"], torch.full((9, 4), low, dtype=torch.float64))


def test_grid_is_bn_grid():
    """bn.hip's bn_grid at the shapes the case list names"""
    assert NR.bn_grid(8300, 8) == (130, 64)          # the finaliser's two-chain loop and its tail
    assert NR.bn_grid(70000, 4) == (1015, 69)        # the 1024 cap: one full trip and a 5-row tail
    assert NR.bn_grid(262200, 4) == (1021, 257)
    assert NR.bn_grid(65, 68) == (2, 33) and NR.bn_grid(64, 64) == (1, 64) and NR.bn_grid(4, 32768) == (1, 4)


_CASES = NR.cases()


def test_restatement_is_within_a_quarter_of_K():
    """the derivation of K: 4 x the worst ratio of the fp32 restatement over every case of the GPU test"""
    worst, bad = {}, []
    for c in _CASES:
        got, ref, S = NR.restate_case(c)
        for k, v in NR.ratios(got, ref, S).items():
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, NR.case_id(c))
            if not v <= NR.K[k] / 4:
                bad.append((NR.case_id(c), k, v))
    for k, (v, cid) in sorted(worst.items()):
        print(f"{k}: worst ratio {v:.3f} ({cid}), K = {NR.K[k]}")
    assert set(worst) == set(NR.K)
    assert not bad, bad[:10]


def test_restatement_masks_are_the_fp64_masks_where_u_is_resolved():
    """the precondition of the mask rule: a correct fp32 implementation has y > 0 where the fp64 u > 0, wherever |u| > K[y] S_y"""
    n = 0
    for c in _CASES:
        if c["act"] in NR.MASKED:
            got, ref, S = NR.restate_case(c)
            assert NR.mask_disagreements(got["y"], ref, S) == 0, NR.case_id(c)
            n += 1
    assert n > 40


MUTATIONS = [
    ("drop_row", dict(kind="bn", B=1, R=70000, C=4)),            # the last row of one 69-row chunk
    ("skip_chunk", dict(kind="bn", B=1, R=8300, C=8)),           # chunk k + 64 in the finaliser
    ("rv_R", dict(kind="bn", B=1, R=17, C=8)),                   # R where R - 1 belongs in running_var
    ("pivot_image", dict(kind="inorm", B=3, R=65, C=68, offset=NR.N.OFFSET)),      # the pivot of image 0 for image 2
    ("k1_sign", dict(kind="bn", B=1, R=65, C=68)),               # the sign of k1 in bn_dx
    ("drop_channel", dict(kind="bn", B=1, R=129, C=132)),        # channel 131
]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("mutate,case", MUTATIONS, ids=[m for m, _ in MUTATIONS])
def test_a_planted_fault_exceeds_K(mutate, case, act):
    c = dict(case, act=act)
    clean = NR.ratios(*NR.restate_case(c))
    assert all(v <= NR.K[k] / 4 for k, v in clean.items()), clean
    r = NR.ratios(*NR.restate_case(c, mutate=mutate))
    over = {k: round(v, 1) for k, v in r.items() if v > NR.K[k]}
    print(f"{mutate} act {act}: over K: {over}")
    assert over, f"{mutate}: no output beyond K: {r}"
