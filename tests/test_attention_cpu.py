"""CPU-side checks of the attention feature: the fp64 reference of tests/attention_ref.py against an independent fp32 evaluation
(the formulas the kernels use: row max, log-sum-exp, dS = P (dP - delta)) inside the GPU tests' bounds, so the case tables are known
to be well conditioned without a GPU; which plan branch each case reaches, pinned to the library's workspace query; the structured
cases' admission rule; the kernels' algorithm restated in fp32 with planted faults, each caught by a named case; the route switch."""
import pytest
import torch

import vae_play_amd
from tests import attention_ref as R
from tests.util import assert_close
from vae_play_amd import _lib, functional


def flash_fp32(inp):
    """fp32, per image, no autograd: P from the log-sum-exp, gradients from delta -- the backward kernels' algebra."""
    q, k, v, x, g, gamma = (inp[n].float() for n in ("q", "k", "v", "x", "g", "gamma"))
    out = {n: [] for n in ("y", "o", "lse", "dq", "dk", "dv")}
    dgamma = torch.zeros(())
    for b in range(q.shape[0]):
        s = q[b] @ k[b].t()
        m = s.max(dim=1, keepdim=True).values
        lse = m + torch.log(torch.exp(s - m).sum(dim=1, keepdim=True))
        p = torch.exp(s - lse)
        o = p @ v[b]
        out["y"].append(gamma * o + x[b])
        out["o"].append(o)
        out["lse"].append(lse[:, 0])
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


@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_reference_matches_independent_fp32(case):
    inp, ref = R.reference(case)
    got = flash_fp32(inp)
    assert_close(got["y"], ref["y"], R.Y_TOL, "fp32 y")
    for n in ("dq", "dk", "dv", "dx"):
        assert_close(got[n], ref[n], R.GRAD_TOL, f"fp32 {n}")
    assert abs(got["dgamma"].double() - ref["dgamma"]).item() <= R.DGAMMA_ABS * ref["abs_go"].item()


def test_tables_keep_their_indices():
    """other tests name CASES[2], [6], [7] and [-1]; BRANCH_CASES is a list of its own so that they keep their meaning"""
    assert len(R.CASES) == 10 and R.CASES[2] == (3, 17, 5, 40, 1, 0) and R.CASES[6] == (2, 65, 12, 100, 1, 0)
    assert R.CASES[7] == (2, 258, 32, 256, 1, 1) and R.CASES[-1] == (2, 130, 8, 64, 4, 0)
    assert len(set(R.ALL_CASES)) == len(R.ALL_CASES) == 19


# what each BRANCH_CASES row is in the table for, as values of R.branches(): dropping or changing a row fails here by its name
BRANCH_OF = {
    (2, 66, 33, 65, 1, 1): dict(ns=2, dq_tail=1, nt_d=8, dchunks=1, nt_c=8, cchunks=1, dp_tail=1, vec_s=0, vec_c=0, last_rows=2),
    (2, 70, 36, 129, 1, 0): dict(ns=2, dq_tail=4, nt_d=8, vec_s=1, nt_c=8, cchunks=2, c_tail=1, dp_tail=1, vec_c=0),
    (1, 130, 64, 128, 1, 1): dict(ns=2, dq_tail=32, vec_s=1, nt_c=8, cchunks=1, c_tail=128, vec_c=1, tiles=3, last_rows=2),
    (2, 129, 40, 72, 1, 1): dict(tiles=3, last_rows=1, vec_s=1, vec_c=1, ns=2, nt_c=8),
    (1, 65, 130, 16, 1, 1): dict(nt_d=8, dchunks=2, d_tail=2, vec_s=0, ns=5, last_rows=1),
    (1, 64, 132, 20, 1, 1): dict(nt_d=8, dchunks=2, d_tail=4, vec_s=1, ns=5, last_rows=64),
    (33, 130, 4, 8, 1, 0): dict(rows=4290, row_blocks=1024, row_strides=True, dgamma_strides=True),
    (1, 193, 8, 64, 4, 0): dict(tiles=4, last_rows=1, nt_c=4, cchunks=1),
    (2, 67, 7, 37, 1, 0): dict(nt_c=4, vec_c=0, nc=2, dp_tail=5, nt_d=2, vec_s=0, last_rows=3),
}


@pytest.mark.parametrize("case", list(BRANCH_OF), ids=R.case_id)
def test_branch_case_reaches_its_branch(case):
    assert case in R.BRANCH_CASES, f"{R.case_id(case)} left BRANCH_CASES"
    br = R.branches(case)
    for name, value in BRANCH_OF[case].items():
        assert br[name] == value, (R.case_id(case), name, br[name], value)


def test_branch_coverage():
    """The union of both tables (and of the VP_ATTN_NT runs of R.NT_CASES) holds every combination the plan can produce: nt_c x
    one / several channel chunks (nt_c = 4 has several only under the knob: the plan gives it C <= 64), nt_d x dchunks (nt_d = 2
    means dq <= 32, a single chunk, so (2, 2) cannot occur), ns in {1, 2, >= 3} x vec_s, both vec_c, a last tile of one row and a
    full one, one-column tails of every chunked width, and the row pass and dgamma both with and without their strides."""
    assert set(BRANCH_OF) == set(R.BRANCH_CASES)
    plain = [R.branches(c) for c in R.ALL_CASES]
    knob = [R.branches(c, nt) for nt, cases in R.NT_CASES.items() for c in cases]
    assert {c[3] for c in R.NT_CASES[4]} == {100, 129, 256, 720} and {c[3] for c in R.NT_CASES[8]} == {8, 40, 64}
    assert {(b["nt_c"], b["cchunks"] > 1) for b in plain} == {(4, False), (8, False), (8, True)}
    assert {(b["nt_c"], b["cchunks"] > 1) for b in plain + knob} == {(4, False), (4, True), (8, False), (8, True)}
    assert max(b["cchunks"] for b in knob) == 12                                     # C = 720 in chunks of 64
    assert {(b["nt_d"], b["dchunks"]) for b in plain} == {(2, 1), (8, 1), (8, 2)}
    assert {(min(b["ns"], 3), b["vec_s"]) for b in plain} == {(n, v) for n in (1, 2, 3) for v in (0, 1)}
    assert {b["vec_c"] for b in plain} == {0, 1}
    assert {(b["nt_d"], b["vec_s"]) for b in plain} == {(2, 0), (2, 1), (8, 0), (8, 1)}      # wstage_load<2> and <8>, each both ways
    assert {(b["nt_c"], b["vec_c"]) for b in plain} == {(4, 0), (4, 1), (8, 0), (8, 1)}
    assert {1, 64} <= {b["last_rows"] for b in plain}
    assert any(b["ns"] > 1 and b["dq_tail"] == 1 for b in plain)
    assert any(b["cchunks"] > 1 and b["c_tail"] == 1 for b in plain)
    assert any(b["nc"] > 1 and b["dp_tail"] == 1 for b in plain)
    assert {b["row_strides"] for b in plain} == {False, True} and {b["dgamma_strides"] for b in plain} == {False, True}
    assert max(b["tiles"] for b in plain) >= 4


def test_workspace_formula_pins_the_restatement():
    """vp_attn_bwd_workspace_bytes is attn_plan's own row_blocks and layout, and needs no device: R.branches must agree on every
    case, and on both sides of the row pass's limit of 1024 workers."""
    ws = _lib.load().vp_attn_bwd_workspace_bytes
    shapes = [c[:4] for c in R.ALL_CASES] + [R.STEP_SHAPE, R.NEG_SHAPE, R.ONE_SHAPE, (65535, 2, 1, 1),
                                             (1, 4095, 1, 1), (1, 4096, 1, 1), (1, 4097, 1, 1), (3, 1, 1, 1), (1, 5, 1, 1)]
    for shape in shapes:
        br = R.branches(shape)
        assert br["ws_bytes"] == 4 * (-(-br["rows"] // 4) * 4 + -(-br["row_blocks"] // 4) * 4)
        assert ws(*shape) == br["ws_bytes"], (shape, ws(*shape), br)


# ---- structured energies: admitted only if an fp32 evaluation sits well inside the bounds the GPU is held to ----------------------------
@pytest.mark.parametrize("name", R.STRUCTURED)
def test_structured_case_is_admitted(name):
    """The one-quarter rule: flash_fp32 (fp32, the kernels' algebra) within a quarter of Y_TOL in y and of every gradient bound of
    R.structured_ratios.  o and lse are outside the rule and only have to be in bound: o = (y - x) / gamma carries the same absolute
    error on a smaller scale, and with |energy| ~ 100 one fp32 rounding of an energy is already 5e-6 of a weight (measured here:
    o at 0.47 of Y_TOL on "up30" and "neg", y at 0.07 and 0.17)."""
    inp, ref = R.structured_reference(name)
    ratios = R.structured_ratios(flash_fp32(inp), ref)
    print(name, {n: f"{v:.3f}" for n, v in ratios.items()})
    assert sorted(ratios) == ["dgamma", "dk", "dq", "dv", "lse", "o", "y"]
    assert R.misses({n: v for n, v in ratios.items() if n not in ("o", "lse")}, 0.25) == [], ratios
    assert R.misses(ratios) == [], ratios


def test_structured_cases_are_what_they_say():
    e = {n: torch.bmm(R.make_structured(n)["q"], R.make_structured(n)["k"].transpose(1, 2)) for n in R.STRUCTURED}
    tile_max = lambda s: [s[:, :, j:j + 64].max().item() for j in range(0, s.shape[2], 64)]      # noqa: E731
    up, down = tile_max(e["up30"]), tile_max(e["down30"])
    assert len(up) == 4 and all(b - a > 25 for a, b in zip(up, up[1:])) and all(a - b > 25 for a, b in zip(down, down[1:]))
    assert e["up01"][0, 0, -1] - e["up01"][0, 0, 0] > 15 and e["down01"][0, 0, 0] - e["down01"][0, 0, -1] > 15
    assert e["neg"].max().item() < -104 and e["neg"].shape[1] == 70
    assert e["one"].shape == (3, 1, 1)
    _, ref = R.structured_reference("one")      # one key: o = v, lse = the energy, dq = dk = 0
    inp = R.make_structured("one")
    assert torch.equal(ref["o"], inp["v"].double()) and bool((ref["dq"] == 0).all()) and bool((ref["dk"] == 0).all())
    assert torch.allclose(ref["lse"], e["one"][:, :, 0].double(), rtol=1e-6)


# ---- the algorithm restated, and the faults it must not have -------------------------------------------------------------------------
def _every_case():
    """(id, inputs, fp64 reference, the ratio function of its bounds) of both tables and the structured cases"""
    for case in R.ALL_CASES:
        yield (R.case_id(case),) + R.reference(case) + (R.table_ratios,)
    for name in R.STRUCTURED:
        yield (name,) + R.structured_reference(name) + (R.structured_ratios,)


def test_restatement_is_inside_every_bound():
    for cid, inp, ref, ratios in _every_case():
        r = ratios(R.tiled_fp32(inp), ref)
        assert {"y", "o", "lse", "dq", "dk", "dv", "dgamma"} <= set(r)
        assert R.misses(r) == [], (cid, r)
    for nt, cases in R.NT_CASES.items():      # the channel-chunk knob changes no arithmetic of the restatement, only its plan
        for case in cases:
            inp, ref = R.reference(case)
            assert R.misses(R.table_ratios(R.tiled_fp32(inp, nt=nt), ref)) == [], (nt, case)


# fault -> the case that exists to catch it, and a quantity that must leave its GPU bound there
CAUGHT_BY = {
    "phantom_zero": ("down30", "y"),
    "mask_after_max": ("neg", "y"),
    "no_alpha": ("up30", "y"),
    "lse_is_m": ("B2_N64_dq8_C64_s1_r1", "lse"),
    "s_drops_tail": ("B2_N66_dq33_C65_s1_r1", "y"),
    "dp_drops_tail": ("B2_N70_dq36_C129_s1_r0", "dq"),
    "dchunk1_unwritten": ("B1_N65_dq130_C16_s1_r1", "dk"),
    "row_pass_stops": ("B33_N130_dq4_C8_s1_r0", "dq"),
    "dgamma_first_256": ("B33_N130_dq4_C8_s1_r0", "dgamma"),
    "delta_without_gamma": ("B3_N17_dq5_C40_s1_r0", "dq"),
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_is_caught_by_its_case(fault):
    """Each fault a tiled online-softmax kernel can have pushes the named quantity of the named case past the bound the GPU is held
    to (a non-finite result counts as past it), while the unfaulted restatement is inside every bound (above)."""
    cases = {c[0]: c[1:] for c in _every_case()}
    cid, name = CAUGHT_BY[fault]
    inp, ref, ratios = cases[cid]
    r = ratios(R.tiled_fp32(inp, fault=fault), ref)
    print(fault, cid, {n: f"{v:.3g}" for n, v in r.items()})
    assert name in R.misses(r), (fault, cid, r)


def test_every_fault_is_planted_and_named():
    assert sorted(CAUGHT_BY) == sorted(R.FAULTS) and len(R.FAULTS) == 10


def test_softmax_faults_escape_the_random_table():
    """Why the structured cases exist: the mask after the max changes nothing that the bounds see on any of the ten random cases
    (a real energy >= 0 is in every row), and the missing alpha rescale nothing on those of one or two key tiles -- it shows on the
    longer ones only because random maxima happen to rise there."""
    for case in R.CASES:
        inp, ref = R.reference(case)
        assert R.misses(R.table_ratios(R.tiled_fp32(inp, fault="mask_after_max"), ref)) == [], case
        if case[1] <= 65:
            assert R.misses(R.table_ratios(R.tiled_fp32(inp, fault="no_alpha"), ref)) == [], case


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
    for B, N, dq, C, _, _ in R.ALL_CASES:
        n = ws(B, N, dq, C)
        assert n >= B * N * 4                                            # delta, one float per row
        if N >= 64:
            assert n < N * N * 4, (B, N, dq, C, n)
        for bigger in ((B + 1, N, dq, C), (B, N + 1, dq, C), (B, N, dq + 1, C), (B, N, dq, C + 1),
                       (4 * B, N, dq, C), (B, 4 * N, dq, C), (B, N, 4 * dq, C), (B, N, dq, 4 * C)):
            assert ws(*bigger) >= n, (bigger, n)
    assert ws(4, 2048, 90, 720) < 2048 * 2048 * 4 // 100
    assert ws(0, 4, 4, 4) == 0 and ws(4, 4, 0, 4) == 0 and ws(1, -1, 1, 1) == 0
