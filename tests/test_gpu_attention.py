"""GPU tests of the flash-style SelfAttentionBlock kernels (csrc/attention.hip) behind functional.self_attention: the case tables of
tests/attention_ref.py (the random cases and the plan-branch cases) against fp64 on both routes, the structured energies that pin the
online softmax, the masking, layout, reproducibility, launch-count and memory conditions, the block itself against the oracle, the
entry points' refusals, guarded runs through the C ABI, unaligned bases, the batch at the grid's bound and the VP_ATTN_NT knob."""
import ctypes
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import vae_play_amd
from tests import attention_ref as R
from tests.guarded import Guards, same_bits
from tests.util import ROOT, assert_close, record
from vae_play_amd import _lib, functional, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("q", "k", "v", "x", "gamma")


@pytest.fixture(autouse=True)
def _route_back_to_auto():
    yield
    vae_play_amd.set_attention_route("auto")
    _lib.TRACE = None


def to4(t):
    """(B, N, c) -> the (B, c, N, 1) channels_last view of the same memory: what the block's maps are to the kernels."""
    B, N, c = t.shape
    return t.view(B, N, 1, c).permute(0, 3, 1, 2)


def to3(t4):
    B, c, H, W = t4.shape
    return t4.permute(0, 2, 3, 1).reshape(B, H * W, c)


def run(inp, route, needs=NAMES, gamma=None, nchw=False):
    """functional.self_attention on the device under ``route``: y and the gradients of the operands named in ``needs``."""
    vae_play_amd.set_attention_route(route)
    t = {n: inp[n].to(DEV) for n in NAMES}
    if gamma is not None:
        t["gamma"] = torch.full((1,), float(gamma), device=DEV)
    a = {n: (to4(t[n]) if n != "gamma" else t[n]).detach() for n in NAMES}
    if nchw:
        a["x"] = a["x"].contiguous()
    for n in needs:
        a[n].requires_grad_(True)
    y = functional.self_attention(a["x"], a["q"], a["k"], a["v"], a["gamma"])
    out = {"y": to3(y.detach())}
    if needs:
        y.backward(to4(inp["g"].to(DEV)))
        for n in needs:
            out["d" + n] = a[n].grad if n == "gamma" else to3(a[n].grad)
    torch.cuda.synchronize()
    return out


def check(out, ref, what):
    assert_close(out["y"], ref["y"], R.Y_TOL, f"{what} y")
    for n in ("dq", "dk", "dv", "dx"):
        if n in out:
            assert_close(out[n], ref[n], R.GRAD_TOL, f"{what} {n}")
    if "dgamma" in out:
        err = abs(out["dgamma"].double().cpu() - ref["dgamma"]).item()
        print(f"{what} dgamma: |err| {err:.3e}, bound {R.DGAMMA_ABS * ref['abs_go'].item():.3e}")
        assert err <= R.DGAMMA_ABS * ref["abs_go"].item(), what


@pytest.mark.parametrize("route", ["fused", "gemm"])
@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_case_table_against_fp64(case, route):
    inp, ref = R.reference(case)
    check(run(inp, route), ref, route)


@pytest.mark.parametrize("case", [R.CASES[2], R.CASES[7]], ids=R.case_id)
def test_gamma_zero(case):
    """The reference's initial gamma (models/blocks.py:73): y is x bit for bit, dq, dk, dv are exactly zero, dgamma is not."""
    inp, _ = R.reference(case)
    zero = dict(inp, gamma=torch.zeros(1))
    ref = R.evaluate(zero)
    out = run(zero, "fused")
    assert torch.equal(out["y"].cpu(), inp["x"])
    for n in ("dq", "dk", "dv"):
        assert bool((out[n] == 0).all()), n
    assert torch.equal(out["dx"].cpu(), inp["g"])
    err = abs(out["dgamma"].double().cpu() - ref["dgamma"]).item()
    assert ref["dgamma"].abs().item() > 0 and err <= R.DGAMMA_ABS * ref["abs_go"].item()


@pytest.mark.parametrize("case", [R.CASES[2], R.CASES[6]], ids=R.case_id)
def test_zero_queries_give_the_mean_of_v(case):
    """q = 0: uniform attention, so o is the per-image mean of v over the N real keys -- a phantom key in the last tile shows here."""
    inp, _ = R.reference(case)
    q, k, v, x, gamma = (inp[n].to(DEV) for n in NAMES)
    _, o, lse = ops.attention_fwd(torch.zeros_like(q), k, v, x, gamma)
    mean = inp["v"].double().mean(dim=1, keepdim=True).expand(-1, case[1], -1)
    assert_close(o, mean, 2e-6, "uniform attention o")
    assert_close(lse, torch.full(tuple(lse.shape), math.log(case[1]), dtype=torch.float64), 2e-6, "uniform attention lse")


@pytest.mark.parametrize("case", [(3, 17, 5, 40, 1, 1), (2, 65, 12, 100, 1, 1)], ids=R.case_id)
def test_strictly_positive_energies(case):
    """ReLU'd q and k shifted by +1: every real energy is > 0, so a key past N left at energy 0 would still get visible weight."""
    inp, ref = R.reference(case, seed=1, shift=1.0)
    assert torch.bmm(inp["q"], inp["k"].transpose(1, 2)).min().item() > 0
    check(run(inp, "fused"), ref, "positive energies")


def test_nchw_and_channels_last_x_give_the_same_bits():
    inp, _ = R.reference(R.CASES[6])
    a, b = run(inp, "fused"), run(inp, "fused", nchw=True)
    for n in a:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("case", [R.CASES[6], R.CASES[7]], ids=R.case_id)
def test_two_runs_give_the_same_bits(case):
    inp, _ = R.reference(case)
    a, b = run(inp, "fused"), run(inp, "fused")
    assert sorted(a) == ["dgamma", "dk", "dq", "dv", "dx", "y"]
    for n in a:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("needs", [("v",), ("q", "k")])
def test_needs_input_grad_subsets(needs):
    inp, ref = R.reference(R.CASES[6])
    out = run(inp, "fused", needs=needs)
    assert sorted(out) == sorted(["y"] + ["d" + n for n in needs])
    check(out, ref, "subset " + "+".join(needs))


def test_no_grad_forward():
    inp, ref = R.reference(R.CASES[6])
    with torch.no_grad():
        out = run(inp, "fused", needs=())
    assert_close(out["y"], ref["y"], R.Y_TOL, "no_grad y")


def _calls(B, route, backward):
    inp = R.make(B, 65, 12, 100)
    vae_play_amd.set_attention_route(route)
    a = {n: (to4(inp[n].to(DEV)) if n != "gamma" else inp[n].to(DEV)).requires_grad_(backward) for n in NAMES}
    g = to4(inp["g"].to(DEV))
    _lib.TRACE = {"events": []}
    try:
        y = functional.self_attention(a["x"], a["q"], a["k"], a["v"], a["gamma"])
        if backward:
            y.backward(g)
        torch.cuda.synchronize()
        return [e[0] for e in _lib.TRACE["events"]]
    finally:
        _lib.TRACE = None


def test_launch_counts():
    fwd = {B: _calls(B, "fused", False) for B in (1, 3)}
    both = {B: _calls(B, "fused", True) for B in (1, 3)}
    assert fwd[1] == fwd[3] == ["vp_attn_fwd_f32"]
    assert both[1] == both[3] and len(both[1]) <= 5 and "vp_attn_bwd_f32" in both[1]
    gemm = {B: len(_calls(B, "gemm", True)) for B in (1, 3)}
    assert gemm[3] > gemm[1] > len(both[1])


def test_memory_stays_below_one_attention_map():
    """A condition, not a measurement: fused forward + backward at N = 2048 raises the peak by less than N*N*4 bytes (one image's
    map) over the inputs and outputs; the GEMM route, which keeps the (B, N, N) map, by more than B*N*N*4."""
    B, N, dq, C = 2, 2048, 8, 64
    inp = R.make(B, N, dq, C)
    extra = {}
    for route in ("fused", "gemm"):
        vae_play_amd.set_attention_route(route)
        a = {n: (to4(inp[n].to(DEV)) if n != "gamma" else inp[n].to(DEV)).requires_grad_(True) for n in NAMES}
        g = to4(inp["g"].to(DEV))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = functional.self_attention(a["x"], a["q"], a["k"], a["v"], a["gamma"])
        y.backward(g)
        torch.cuda.synchronize()
        grads = {a[n].grad.data_ptr(): a[n].grad.numel() * 4 for n in NAMES if a[n].grad.data_ptr() != g.data_ptr()}      # dx may be g itself
        outputs = y.numel() * 4 + sum(grads.values())
        extra[route] = torch.cuda.max_memory_allocated() - base - outputs
        del y, a, g
    print(f"peak over inputs and outputs: fused {extra['fused']} B, gemm {extra['gemm']} B, one map {N * N * 4} B")
    assert extra["fused"] < N * N * 4
    assert extra["gemm"] > B * N * N * 4


@pytest.mark.parametrize("channels,hw", [(40, (3, 5)), (256, (258, 1))])
def test_block_matches_oracle(channels, hw):
    """SelfAttentionBlock end to end (1x1 projections + attention) against the oracle, at the bounds of
    tests/test_gpu_font.py::test_self_attention_block_matches_oracle."""
    from oracle import ref_font as FN
    from vae_play_amd.blocks import SelfAttentionBlock
    torch.manual_seed(2)
    blk = SelfAttentionBlock(channels)
    with torch.no_grad():
        blk.gamma.fill_(0.7)
    p = {"a." + k: v.detach().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
    blk = blk.to(DEV)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, channels, *hw, generator=g)
    gy = torch.randn(2, channels, *hw, generator=g)
    xo = x.clone().requires_grad_(True)
    yo = FN.self_attention(p, "a.", xo)
    yo.backward(gy)
    xd = x.to(DEV).requires_grad_(True)
    vae_play_amd.set_attention_route("fused")
    _lib.TRACE = {"events": []}
    y = blk(xd)
    names = [e[0] for e in _lib.TRACE["events"]]
    _lib.TRACE = None
    assert names.count("vp_attn_fwd_f32") == 1 and "vp_gemm_f32" not in names
    y.backward(gy.to(DEV))
    assert_close(y, yo.detach(), 2e-5, "block y")
    assert_close(xd.grad, xo.grad, 5e-5, "block dx")
    for n, q in blk.named_parameters():
        assert_close(q.grad, p["a." + n].grad, 1e-4, f"block grad {n}")


def _args(B=2, N=17, dq=5, C=40):
    inp = R.make(B, N, dq, C)
    t = {n: inp[n].to(DEV) for n in ("q", "k", "v", "x", "g", "gamma")}
    t["y"], t["o"] = torch.full_like(t["x"], 7.0), torch.full_like(t["x"], 7.0)
    t["lse"] = torch.full((B, N), 7.0, device=DEV)
    t["dq"], t["dk"], t["dv"] = torch.full_like(t["q"], 7.0), torch.full_like(t["k"], 7.0), torch.full_like(t["v"], 7.0)
    t["dgamma"] = torch.full((1,), 7.0, device=DEV)
    t["ws"] = torch.full((max(1, ops.attention_bwd_workspace_bytes(B, N, dq, C) // 4),), 7.0, device=DEV)
    return t


def _fwd(t, dims, null=None):
    p = [None if n == null else ops._p(t[n]) for n in ("q", "k", "v", "x", "gamma", "y", "o", "lse")]
    _lib.call("vp_attn_fwd_f32", *p, *dims, ops._stream())


def _bwd(t, dims, null=None, ws_bytes=None):
    p = [None if n == null else ops._p(t[n]) for n in ("q", "k", "v", "o", "lse", "g", "gamma", "dq", "dk", "dv", "dgamma", "ws")]
    _lib.call("vp_attn_bwd_f32", *p, ctypes.c_size_t(t["ws"].numel() * 4 if ws_bytes is None else ws_bytes), *dims, ops._stream())


def _untouched(t):
    torch.cuda.synchronize()
    return all(bool((t[n] == 7.0).all()) for n in ("y", "o", "lse", "dq", "dk", "dv", "dgamma", "ws"))


def test_abi_refusals_launch_nothing():
    dims = (2, 17, 5, 40)
    t = _args(*dims)
    bad_dims = [tuple(0 if i == j else d for i, d in enumerate(dims)) for j in range(4)]
    bad_dims += [(-1, 17, 5, 40), (65536, 17, 5, 40),
                 (1, 1 << 20, 5, 1 << 12), (1, 1 << 24, 1 << 8, 40)]      # N * max(C, dq) = 2^32: past the 32-bit in-image index
    for d in bad_dims:
        with pytest.raises(_lib.VaePlayHipError):
            _fwd(t, d)
        with pytest.raises(_lib.VaePlayHipError):
            _bwd(t, d)
    for n in ("q", "k", "v", "x", "gamma", "y", "o", "lse"):
        with pytest.raises(_lib.VaePlayHipError):
            _fwd(t, dims, null=n)
    for n in ("q", "k", "v", "o", "lse", "g", "gamma", "dgamma", "ws"):
        with pytest.raises(_lib.VaePlayHipError):
            _bwd(t, dims, null=n)
    need = ops.attention_bwd_workspace_bytes(*dims)
    with pytest.raises(_lib.VaePlayHipError, match="workspace"):
        _bwd(t, dims, ws_bytes=need - 4)
    assert _untouched(t)
    # and the same arguments, unrefused, do run: null dq / dk / dv are the optional ones
    _fwd(t, dims)
    _bwd(t, dims, null="dq")
    torch.cuda.synchronize()
    assert bool((t["dq"] == 7.0).all()) and not bool((t["dk"] == 7.0).any()) and not bool((t["y"] == 7.0).any())


# ---- the fused kernels through ops / the C ABI: what functional.self_attention does not let through (N = 1) or does not show -------------
OUTS = ("y", "o", "lse", "dq", "dk", "dv", "dgamma")


def fused(t):
    """ops.attention_fwd + attention_bwd on device operands: every output of the two entry points"""
    y, o, lse = ops.attention_fwd(t["q"], t["k"], t["v"], t["x"], t["gamma"])
    d_q, d_k, d_v, dgamma = ops.attention_bwd(t["q"], t["k"], t["v"], o, lse, t["g"], t["gamma"])
    torch.cuda.synchronize()
    return dict(zip(OUTS, (y, o, lse, d_q, d_k, d_v, dgamma)))


def on_device(inp):
    return {n: inp[n].to(DEV) for n in ("q", "k", "v", "x", "g", "gamma")}


def held(ratios, what):
    """every error / bound recorded and printed, then all of them finite and <= 1"""
    for n, v in ratios.items():
        record(f"{what} {n} / bound", v)
    print(what, {n: f"{v:.3g}" for n, v in ratios.items()})
    assert R.misses(ratios) == [], (what, ratios)


@pytest.mark.parametrize("name", R.STRUCTURED)
def test_structured_energies(name):
    """Energies whose maximum moves where the case says (tests/attention_ref.py: up / down per key tile and per key, all far below
    zero, one key): y, o, lse at Y_TOL, the gradients at GRAD_TOL times their fp64 conditioning.  tests/test_attention_cpu.py shows
    which planted fault of the online softmax each one catches."""
    inp, ref = R.structured_reference(name)
    got = fused(on_device(inp))
    for n in OUTS:
        assert bool(torch.isfinite(got[n]).all()), n
    held(R.structured_ratios(got, ref), f"structured {name}")
    if name == "one":      # p = exp(0) = 1 for the one real key, 0 for the 63 phantom ones, l = 1: nothing rounds
        assert torch.equal(got["o"].cpu(), inp["v"])


@pytest.mark.parametrize("case", [R.BRANCH_CASES[0], R.BRANCH_CASES[6], R.BRANCH_CASES[4]], ids=R.case_id)
def test_guarded_abi(case):
    """vp_attn_fwd_f32 / vp_attn_bwd_f32 with every output between sentinels and a workspace of exactly the queried size: nothing
    is stored past row N of the last image or past the workspace's partials, nothing is left unwritten, the values are the table's,
    and a second call gives the same bits."""
    assert R.BRANCH_CASES[0][:4] == (2, 66, 33, 65) and R.BRANCH_CASES[6][:4] == (33, 130, 4, 8) and R.BRANCH_CASES[4][:4] == (1, 65, 130, 16)
    dims = B, N, dq, C = case[:4]
    inp, ref = R.reference(case)
    src = on_device(inp)

    def once():
        G = Guards(DEV)
        t = dict(src, y=G.out("y", B, N, C), o=G.out("o", B, N, C), lse=G.out("lse", B, N), dq=G.out("dq", B, N, dq),
                 dk=G.out("dk", B, N, dq), dv=G.out("dv", B, N, C), dgamma=G.out("dgamma", 1))
        t["ws"], nbytes = G.ws("ws", int(_lib.load().vp_attn_bwd_workspace_bytes(*dims)))
        assert nbytes == R.branches(case)["ws_bytes"] == t["ws"].numel() * 4
        _fwd(t, dims)
        _bwd(t, dims, ws_bytes=nbytes)
        G.check()
        return {n: t[n] for n in OUTS}

    a, b = once(), once()
    held(R.table_ratios(a, ref), "guarded")
    for n in OUTS:
        assert same_bits(a[n], b[n]), n


def _one_float_in(t):
    """a contiguous copy of t that starts 4 bytes into a larger allocation: not 16-byte aligned"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("case", [R.CASES[6], R.BRANCH_CASES[2]], ids=R.case_id)
def test_unaligned_bases_give_the_same_bits(case):
    """dq % 4 == 0 and C % 4 == 0, so aligned bases take the 16-byte loads of load_run; with q, k, v, g starting one float into
    their allocations the launchers must fall back to four 4-byte loads, which feed the same values into the same summation
    order: every output equal bit for bit.  This checks the fall-back's arithmetic and that it is taken without a fault here; it
    does not check that the hardware would refuse an unaligned 16-byte load."""
    assert case[2] % 4 == 0 and case[3] % 4 == 0 and R.branches(case)["vec_s"] == R.branches(case)["vec_c"] == 1
    src = on_device(R.reference(case)[0])
    assert all(src[n].data_ptr() % 16 == 0 for n in ("q", "k", "v", "g"))
    a = fused(src)
    b = fused(dict(src, **{n: _one_float_in(src[n]) for n in ("q", "k", "v", "g")}))
    for n in OUTS:
        assert same_bits(a[n], b[n]), n
    held(R.table_ratios(a, R.reference(case)[1]), "aligned")


def test_batch_at_the_grid_bound():
    """B = 65535 is the largest batch attn_check_dims lets through (the grid's z); test_abi_refusals_launch_nothing refuses 65536"""
    case = (65535, 2, 1, 1, 1, 0)
    inp, ref = R.reference(case)
    got = fused(on_device(inp))
    held(R.table_ratios(got, ref), "B = 65535")


def test_attn_nt_knob():
    """VP_ATTN_NT forces the channel chunk of forward / dV: chunks of 64 on C = 100, 129, 256, 720 (up to 12
    chunks) and chunks of 128 on C = 8, 40, 64, plus the plan's own choice.  One fresh child process (the knob is read per launch
    only with VP_ENV_DYNAMIC=1 set before the library loads) runs the fused kernels against fp64 and prints error / bound.
    A column's arithmetic does not depend on the chunk it falls in, so the forced runs must also equal the plan's own bit for bit --
    and a knob that was silently ignored would pass all of this: what is held is that either chunking of every C gives finite,
    in-bound, identical results, not which one ran."""
    env = dict(os.environ, VP_ENV_DYNAMIC="1")
    env.pop("VP_ATTN_NT", None)
    r = subprocess.run([sys.executable, "-m", "tests.attention_ref"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    want = {"4": R.NT_CASES[4], "8": R.NT_CASES[8], "unset": R.NT_CASES[4] + R.NT_CASES[8]}
    same = res.pop("same_bits")
    assert sorted(res) == sorted(want)
    assert sorted(same) == sorted(f"{k} {R.case_id(c)}" for k in ("4", "8") for c in R.NT_CASES[int(k)]) and all(same.values()), same
    for knob, cases in want.items():
        assert sorted(res[knob]) == sorted(R.case_id(c) for c in cases), knob
        for cid, ratios in res[knob].items():
            assert sorted(ratios) == sorted(OUTS)
            held(ratios, f"VP_ATTN_NT {knob} {cid}")
