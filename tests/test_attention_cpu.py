"""CPU-side checks of the attention feature: the fp64 reference of tests/attention_ref.py against an independent fp32 evaluation
(the formulas the kernels use: row max, log-sum-exp, dS = P (dP - delta)) inside the GPU tests' bounds, so the case table is known
to be well conditioned without a GPU; the route switch; the workspace query, which needs no device."""
import pytest
import torch

import vae_play_amd
from tests import attention_ref as R
from tests.util import assert_close
from vae_play_amd import _lib, functional


def flash_fp32(inp):
    """fp32, per image, no autograd: P from the log-sum-exp, gradients from delta -- the backward kernels' algebra."""
    q, k, v, x, g, gamma = (inp[n].float() for n in ("q", "k", "v", "x", "g", "gamma"))
    out = {n: [] for n in ("y", "dq", "dk", "dv")}
    dgamma = torch.zeros(())
    for b in range(q.shape[0]):
        s = q[b] @ k[b].t()
        m = s.max(dim=1, keepdim=True).values
        lse = m + torch.log(torch.exp(s - m).sum(dim=1, keepdim=True))
        p = torch.exp(s - lse)
        o = p @ v[b]
        out["y"].append(gamma * o + x[b])
        dgamma = dgamma + (g[b] * o).sum()
        do = gamma * g[b]
        delta = (do * o).sum(dim=1, keepdim=True)
        ds = p * (do @ v[b].t() - delta)
        out["dv"].append(p.t() @ do)
        out["dq"].append(ds @ k[b])
        out["dk"].append(ds.t() @ q[b])
    res = {n: torch.stack(t) for n, t in out.items()}
    res["dx"], res["dgamma"] = g, dgamma.reshape(1)
    return res


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_reference_matches_independent_fp32(case):
    inp, ref = R.reference(case)
    got = flash_fp32(inp)
    assert_close(got["y"], ref["y"], R.Y_TOL, "fp32 y")
    for n in ("dq", "dk", "dv", "dx"):
        assert_close(got[n], ref[n], R.GRAD_TOL, f"fp32 {n}")
    assert abs(got["dgamma"].double() - ref["dgamma"]).item() <= R.DGAMMA_ABS * ref["abs_go"].item()


def test_last_case_overflows_without_the_max():
    inp, _ = R.reference(R.CASES[-1])
    s = torch.bmm(inp["q"], inp["k"].transpose(1, 2))
    assert s.max().item() > 89.0 and not torch.isfinite(torch.exp(s)).all()


def test_auto_route():
    """The measured winners (profiles/r12_attention.json, forward + backward), which the rule must reproduce."""
    assert functional.attention_route_for(16, 258, 32, 256) == "fused"      # networks_BC.RefineNet: 7x faster fused
    assert functional.attention_route_for(4, 2048, 90, 720) == "gemm"       # networks_BP.ValueEncoder: fused takes 2x the time
    assert functional.attention_route_for(2, 1, 4, 32) == "gemm"            # N = 1: the short-circuit, on every route
    for B, C, N, winner in ((16, 256, 512, "fused"), (16, 256, 1024, "fused"), (4, 256, 2048, "gemm"), (4, 720, 512, "gemm"),
                            (4, 720, 1024, "gemm"), (1, 720, 2048, "gemm"), (2, 32, 16, "fused")):
        assert functional.attention_route_for(B, N, C // 8, C) == winner, (B, C, N)
    for hw in ((4, 4), (3, 5)):                                              # the block's existing GPU test shapes run fused
        assert functional.attention_route_for(2, hw[0] * hw[1], 4, 32) == "fused"


def test_set_attention_route():
    assert vae_play_amd.get_attention_route() == "auto"
    try:
        for r in ("fused", "gemm", "auto"):
            vae_play_amd.set_attention_route(r)
            assert vae_play_amd.get_attention_route() == r
        with pytest.raises(ValueError):
            vae_play_amd.set_attention_route("flash")
        assert vae_play_amd.get_attention_route() == "auto"
    finally:
        vae_play_amd.set_attention_route("auto")


def test_workspace_query_needs_no_device():
    ws = _lib.load().vp_attn_bwd_workspace_bytes
    for B, N, dq, C, _, _ in R.CASES:
        n = ws(B, N, dq, C)
        assert n >= B * N * 4                                            # delta, one float per row
        if N >= 64:
            assert n < N * N * 4, (B, N, dq, C, n)
        for bigger in ((B + 1, N, dq, C), (B, N + 1, dq, C), (B, N, dq + 1, C), (B, N, dq, C + 1),
                       (4 * B, N, dq, C), (B, 4 * N, dq, C), (B, N, 4 * dq, C), (B, N, dq, 4 * C)):
            assert ws(*bigger) >= n, (bigger, n)
    assert ws(4, 2048, 90, 720) < 2048 * 2048 * 4 // 100
    assert ws(0, 4, 4, 4) == 0 and ws(4, 4, 0, 4) == 0 and ws(1, -1, 1, 1) == 0
