"""Scoring on the fused inference plan (FusedVAEInference.score), checked without a GPU: the fp64 restatements of tests/score_ref.py
against torch's own functions, the ABI table, and the structure of the lazily built scoring lists over host buffers
(``_plan_only=True``; nothing is run)."""
import gc
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import score_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import gen_golden_fused_plans as G  # noqa: E402  (the canonical form of a launch list)

SCORE_SYMBOLS = ("vp_bce_rows_workspace_bytes", "vp_bce_rows_f32", "vp_latent_iw_fwd_f32", "vp_iw_bound_f32")
CASES = [(prec, C, S, z, B) for prec in ("bf16x3", "f32") for (C, S, z, B) in ((1, 32, 16, 4), (3, 64, 64, 4))]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the references -----------------------------------------------------------------------------------------------------------
def test_ref_bce_rows_is_torchs_bce():
    g = _gen(1)
    p, t = torch.rand(5, 3, 7, generator=g, dtype=torch.float64) * 0.98 + 0.01, torch.rand(5, 3, 7, generator=g, dtype=torch.float64)
    p[0, 0, 0], p[0, 0, 1], t[0, 0, 0], t[0, 0, 1] = 0.0, 1.0, 0.25, 0.75        # the -100 clamp, both sides
    want = F.binary_cross_entropy(p.reshape(5, -1), t.reshape(5, -1), reduction="none").sum(1)
    torch.testing.assert_close(R.bce_rows(p, t), want, rtol=1e-13, atol=0)
    assert R.bce_rows(p, t)[0] > 50.0          # 0.25 * 100 + (1 - 0.75) * 100 from the two clamped elements


def test_ref_latent_iw_is_the_two_gaussian_log_densities():
    g = _gen(2)
    mu, logvar, eps = (torch.randn(6, 9, generator=g, dtype=torch.float64) for _ in range(3))
    z, kl, lr, scale = R.latent_iw(mu, logvar, eps)
    std = torch.exp(0.5 * logvar)
    torch.testing.assert_close(z, mu + std * eps, rtol=1e-14, atol=0)
    log_p = torch.distributions.Normal(torch.zeros_like(z), torch.ones_like(z)).log_prob(z).sum(1)
    log_q = torch.distributions.Normal(mu, std).log_prob(z).sum(1)
    torch.testing.assert_close(lr, log_p - log_q, rtol=1e-12, atol=1e-12)
    want_kl = torch.distributions.kl_divergence(torch.distributions.Normal(mu, std),
                                                torch.distributions.Normal(torch.zeros_like(mu), torch.ones_like(mu))).sum(1)
    torch.testing.assert_close(kl, want_kl, rtol=1e-12, atol=1e-12)
    assert (scale >= lr.abs()).all()


def test_ref_iw_bound_is_logsumexp():
    g = _gen(3)
    nbce = 2e3 + 30.0 * torch.rand(4, 7, generator=g, dtype=torch.float64)
    lr = torch.randn(4, 7, generator=g, dtype=torch.float64)
    logw, iwae = R.iw_bound(nbce, lr)
    torch.testing.assert_close(logw, lr - nbce, rtol=0, atol=0)
    torch.testing.assert_close(iwae, torch.logsumexp(logw, 1) - math.log(7), rtol=1e-14, atol=0)
    assert torch.equal(R.iw_bound(nbce[:, :1], lr[:, :1])[1], logw[:, 0])


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_table_carries_the_scoring_entry_points():
    from vae_play_amd import _lib
    lib = _lib.load()
    for name in SCORE_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the documented bound: rows x ceil(n / 4096) floats
    assert lib.vp_bce_rows_workspace_bytes(3, 1) == 12 and lib.vp_bce_rows_workspace_bytes(3, 4096) == 12
    assert lib.vp_bce_rows_workspace_bytes(3, 4097) == 24 and lib.vp_bce_rows_workspace_bytes(32, 49152) == 32 * 12 * 4


# ---- the plan -----------------------------------------------------------------------------------------------------------------
def _build(prec, C, S, z, B):
    import vae_play_amd as V
    torch.manual_seed(0)
    vae = V.VAE(S, z, C)
    return vae, V.FusedVAEInference(vae, B, S, C, precision=prec, _plan_only=True)


def _record(vae, inf, which):
    """canonical form of the lists ``which`` of a plan (pointers as [owner, ordinal, offset]) and the number of pointers nobody owns"""
    plans, seen = [("prep", inf._prep)], {}
    for w in which:
        for p in inf._plans[w]:
            seen.setdefault(id(p), (p, []))[1].append(w)
    plans += [("+".join(names), p) for p, names in seen.values()]
    calls, unknown, _ = G.canonical(inf, plans, [("", vae)], {})
    return calls, unknown


OLD = ("encode", "decode", "reconstruct")


@pytest.mark.parametrize("prec,C,S,z,B", CASES)
def test_a_plan_that_never_scores_is_untouched(prec, C, S, z, B):
    vae, plain = _build(prec, C, S, z, B)
    assert plain._score is None and set(plain._plans) == set(OLD)
    assert not any(n.startswith("score") for n in plain._bufs)
    _, scored = _build(prec, C, S, z, B)      # (the same seed: the same model)
    before = {n: (tuple(t.shape), t.dtype) for n, t in scored._bufs.items()}
    assert before == {n: (tuple(t.shape), t.dtype) for n, t in plain._bufs.items()} and list(before) == list(plain._bufs)
    lists_before = {w: [id(p) for p in scored._plans[w]] for w in OLD}
    scored.enable_scoring(3)
    scored._score_list(1)
    scored._score_list(3)
    # the old buffers are the same tensors, the old lists the same objects with the same launches; what is new is named score.*
    assert {n: (tuple(t.shape), t.dtype) for n, t in scored._bufs.items() if not n.startswith("score.")} == before
    assert [n for n in scored._bufs if not n.startswith("score.")] == list(before)
    assert {w: [id(p) for p in scored._plans[w]] for w in OLD} == lists_before
    assert set(scored._plans) == set(OLD) | {"score1", "score3"}


@pytest.mark.parametrize("prec,C,S,z,B", CASES)
def test_the_old_lists_have_the_same_launches_after_enabling(prec, C, S, z, B):
    """two builds over the same model, one of them scoring: encode / decode / reconstruct are launch for launch, argument for
    argument the same in the canonical form (buffers by order of first appearance)"""
    import vae_play_amd as V
    torch.manual_seed(0)
    vae = V.VAE(S, z, C)
    plain = V.FusedVAEInference(vae, B, S, C, precision=prec, _plan_only=True)
    scored = V.FusedVAEInference(vae, B, S, C, precision=prec, _plan_only=True)
    scored.enable_scoring(2)
    scored._score_list(2)
    gc.collect()
    want, got = _record(vae, plain, OLD), _record(vae, scored, OLD)
    assert want[1] == 0 and got[1] == 0
    assert got[0] == want[0]
    bytes_of = lambda inf: sum(t.numel() * t.element_size() for n, t in inf._bufs.items() if not n.startswith("score."))   # noqa: E731
    assert bytes_of(scored) == bytes_of(plain)


@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("prec,C,S,z,B", CASES)
def test_scoring_list(prec, C, S, z, B, k):
    from vae_play_amd import _lib
    vae, inf = _build(prec, C, S, z, B)
    inf.enable_scoring(k)
    which = inf._score_list(k)
    assert which == f"score{k}" and inf._score_list(k) == which
    names = lambda w: [c[0] for p in inf._plans[w] for c in p.calls]      # noqa: E731
    # [draw][image] -> [image][draw] for the bound: two launches of the transpose kernel, none for one draw
    tail = ["vp_nchw_to_nhwc_f32"] * 2 * (k > 1) + ["vp_iw_bound_f32"]
    assert names(which) == names("encode") + k * (["vp_latent_iw_fwd_f32"] + names("decode") + ["vp_bce_rows_f32"]) + tail
    # the encoder and decoder lists are the plan's own, not copies
    assert inf._plans[which][0] is inf._plans["encode"][0]
    assert sum(p is inf._plans["decode"][0] for p in inf._plans[which]) == k
    for p in inf._plans[which]:
        for c in p.calls:
            assert len(c[2]) == len(_lib.SIGNATURES[c[0]][1]) and c[6] is None, c[0]
    gc.collect()
    calls, unknown = _record(vae, inf, [which])
    assert unknown == 0, [c[:2] for c in calls if any(isinstance(a, list) and a[:1] == ["?"] for a in c[2])]
    new = [c for c in calls if c[1] in ("vp_latent_iw_fwd_f32", "vp_bce_rows_f32", "vp_iw_bound_f32")]
    assert len(new) == 2 * k + 1
    lat = [c for c in new if c[1] == "vp_latent_iw_fwd_f32"]
    assert [c[2][4] is not None for c in lat] == [True] + [False] * (k - 1)        # kl is written by the first draw alone
    assert len({tuple(c[2][2]) for c in lat}) == k and len({tuple(c[2][5]) for c in lat}) == k      # a draw's own eps and lr
    bce = [c for c in new if c[1] == "vp_bce_rows_f32"]
    assert all(c[2][2:4] == [B, C * S * S] for c in bce) and len({tuple(c[2][4]) for c in bce}) == k
    assert all(c[2][6] >= _lib.load().vp_bce_rows_workspace_bytes(B, C * S * S) for c in bce)
    assert new[-1][2][2:4] == [B, k]


def test_asking_for_more_draws_replaces_the_scoring_buffers_only():
    vae, inf = _build("bf16x3", 1, 32, 16, 4)
    inf.enable_scoring(2)
    inf._score_list(2)
    old = {n: t.data_ptr() for n, t in inf._bufs.items() if not n.startswith("score.")}
    inf.enable_scoring(1)                                   # no shrinking
    assert inf._score.k_max == 2 and "score2" in inf._plans
    inf.enable_scoring(5)
    assert inf._score.k_max == 5 and set(inf._plans) == set(OLD)       # the lists over the old buffers are gone
    assert {n: t.data_ptr() for n, t in inf._bufs.items() if not n.startswith("score.")} == old
    assert inf._bufs["score.eps"].shape == (5, 4, 16)
    with pytest.raises(ValueError):
        inf.enable_scoring(0)


def test_score_refuses_bad_arguments():
    from vae_play_amd import _lib
    vae, inf = _build("bf16x3", 1, 32, 16, 4)
    with pytest.raises(_lib.VaePlayHipError, match="HIP device"):
        inf.score(torch.zeros(2, 1, 32, 32))
    assert inf._score is None                               # a refused call allocates nothing
