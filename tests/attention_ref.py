"""The fp64 statement of SelfAttentionBlock's core on (B, N, .) operands, y = gamma * softmax(q k^T) v + x, in plain torch with
autograd for the gradients; the input maker and the case tables that tests/test_attention_cpu.py and tests/test_gpu_attention.py
share: ten random cases, the plan-branch cases with ``branches`` (attn_plan restated), structured energies with their conditioning-
aware gradient bounds, and ``tiled_fp32``, the kernels' algorithm in fp32 with planted faults.  Run as a module it is the child
process of test_attn_nt_knob."""
import torch

# (B, N, dq, C, scale, relu): N one below, at and above the kernels' 64-row tile (and 16, the MFMA tile); dq not a multiple of the
# MFMA depth 4; C across a channel chunk (64 / 128); the last case has |energy| up to ~230, so exp overflows fp32 without the max
CASES = [
    (2, 2, 1, 8, 1, 0),
    (2, 15, 4, 32, 1, 1),
    (3, 17, 5, 40, 1, 0),
    (1, 16, 4, 32, 1, 1),
    (2, 63, 3, 24, 1, 0),
    (2, 64, 8, 64, 1, 1),
    (2, 65, 12, 100, 1, 0),
    (2, 258, 32, 256, 1, 1),
    (1, 70, 90, 720, 1, 1),
    (2, 130, 8, 64, 4, 0),
]

Y_TOL = 2e-5          # tests/util.OP_RTOL
GRAD_TOL = 5e-5       # dq, dk, dv, dx: the bounds of tests/test_gpu_font.py::test_self_attention_block_matches_oracle
DGAMMA_ABS = 1e-5     # |dgamma - ref| <= DGAMMA_ABS * sum |g o|: a cancelling sum of B N C terms


def case_id(case):
    return "B{}_N{}_dq{}_C{}_s{}_r{}".format(*case)


def make(B, N, dq, C, scale=1, relu=0, seed=0, shift=0.0):
    """fp32 CPU operands: q, k = scale * randn (then ReLU if asked, then + shift), v, x, g = randn, gamma = 0.7."""
    gen = torch.Generator().manual_seed(1000 + seed)
    q = scale * torch.randn(B, N, dq, generator=gen)
    k = scale * torch.randn(B, N, dq, generator=gen)
    if relu:
        q, k = torch.relu(q), torch.relu(k)
    q, k = q + shift, k + shift
    v, x, g = (torch.randn(B, N, C, generator=gen) for _ in range(3))
    return {"q": q, "k": k, "v": v, "x": x, "g": g, "gamma": torch.full((1,), 0.7)}


def evaluate(inp, dtype=torch.float64):
    """y, o, lse and the five gradients of sum(y * g), in ``dtype`` on the CPU, by autograd on the plain statement."""
    q, k, v, x, gamma = (inp[n].to(dtype).clone().requires_grad_(True) for n in ("q", "k", "v", "x", "gamma"))
    g = inp["g"].to(dtype)
    energy = torch.bmm(q, k.transpose(1, 2))
    att = torch.softmax(energy, dim=-1)
    o = torch.bmm(att, v)
    y = gamma * o + x
    y.backward(g)
    return {"y": y.detach(), "o": o.detach(), "lse": torch.logsumexp(energy.detach(), dim=-1),
            "dq": q.grad, "dk": k.grad, "dv": v.grad, "dx": x.grad, "dgamma": gamma.grad, "abs_go": (g * o.detach()).abs().sum()}


_REF = {}


def reference(case, seed=0, shift=0.0):
    """(inputs, fp64 results) of a table case, computed once per session and shared; callers must not modify either."""
    key = (tuple(case), seed, shift)
    if key not in _REF:
        inp = make(*case, seed=seed, shift=shift)
        _REF[key] = (inp, evaluate(inp))
    return _REF[key]


# ---- the plan branches --------------------------------------------------------------------------------------------------------------
# A second table, kept apart so that CASES[-1] keeps its meaning: each row is there for a branch of attn_plan (csrc/attention.h), of
# the launchers' vec_s / vec_c rules or of the row pass that CASES does not reach; ``branches`` states which, and
# tests/test_attention_cpu.py::test_branch_coverage fails by name if a row that carries one is dropped.
BRANCH_CASES = [
    (2, 66, 33, 65, 1, 1),      # ns = 2 with a one-column tail, nt_d = 8, nt_c = 8 at its first C, scalar loads on both operands
    (2, 70, 36, 129, 1, 0),     # 16-byte S loads across two chunks, wstage_load<8> vectorised, C: chunk tails of one column, scalar
    (1, 130, 64, 128, 1, 1),    # two full dq chunks vectorised, exactly one full 128-channel chunk, three key tiles
    (2, 129, 40, 72, 1, 1),     # the last tile holds one row; vector loads on both operands
    (1, 65, 130, 16, 1, 1),     # dchunks = 2 with a two-column tail, scalar
    (1, 64, 132, 20, 1, 1),     # dchunks = 2, vectorised
    (33, 130, 4, 8, 1, 0),      # 4290 rows: the row pass strides, 1024 partials, dgamma's strided sum
    (1, 193, 8, 64, 4, 0),      # |energy| up to ~280 over four tiles, the last of one row
    (2, 67, 7, 37, 1, 0),       # nt_c = 4 with scalar loads (C <= 64, C % 4 != 0): wstage_load<4> unvectorised, dP tail of 5 columns
]
ALL_CASES = CASES + BRANCH_CASES

# VP_ATTN_NT: the channel-chunk width forced to 4 or 8 tiles, on the cases where that is not the plan's choice
NT_CASES = {4: [c for c in ALL_CASES if c[3] in (100, 129, 256, 720)], 8: [c for c in ALL_CASES if c[3] in (8, 40, 64)]}

TILE, DK, MAX_PARTIALS = 64, 32, 1024      # kAttnTile, kAttnDK, kAttnMaxPartials


def _round4(n):
    return (n + 3) // 4 * 4


def branches(case, nt=None):
    """attn_plan and the launchers' vec rules for 16-byte-aligned bases, restated: which path of which kernel a case takes."""
    B, N, dq, C = case[:4]
    tiles = -(-N // TILE)
    ns = -(-dq // DK)
    nt_c = nt if nt in (4, 8) else (4 if C <= 64 else 8)
    cchunks = -(-C // (16 * nt_c))
    nt_d = 2 if dq <= 32 else 8
    dchunks = -(-dq // (16 * nt_d))
    rows = B * N
    row_blocks = min(-(-rows // 4), MAX_PARTIALS)
    return {
        "tiles": tiles, "last_rows": N - TILE * (tiles - 1),
        "ns": ns, "dq_tail": dq - DK * (ns - 1),                              # columns in the last 32-column chunk of S's contraction
        "nt_c": nt_c, "cchunks": cchunks, "c_tail": C - 16 * nt_c * (cchunks - 1),     # channels of the last forward / dV workgroup
        "nc": -(-C // DK), "dp_tail": C - DK * (-(-C // DK) - 1),               # dP's contraction in dK / dQ
        "nt_d": nt_d, "dchunks": dchunks, "d_tail": dq - 16 * nt_d * (dchunks - 1),
        "vec_s": int(dq % 4 == 0), "vec_c": int(C % 4 == 0),
        "rows": rows, "row_blocks": row_blocks, "row_strides": rows > 4 * row_blocks, "dgamma_strides": row_blocks > 256,
        "ws_bytes": 4 * (_round4(rows) + _round4(row_blocks)),
    }


# ---- structured energies ------------------------------------------------------------------------------------------------------------
# q[..., 0] = 1, k[..., 0] = f(key index) and 0.3 x the random columns elsewhere: the energy of key j is f(j) plus noise of ~0.2, the
# same for every query, so WHERE the running maximum moves during the key sweep is chosen, not left to the random draw.
STEP_SHAPE, NEG_SHAPE, ONE_SHAPE = (2, 200, 6, 24), (2, 70, 8, 24), (3, 1, 4, 16)
_STEPS = {
    "up30": lambda j: 30.0 * (j // TILE),        # the maximum rises by 30 at every key tile: alpha = e^-30 each time
    "up01": lambda j: 0.1 * j,                   # ... and inside every tile
    "down30": lambda j: -30.0 * (j // TILE),     # the last tile's 8 real keys sit 90 below the first tile's: 56 phantoms at 0 would rule
    "down01": lambda j: -0.1 * j,
}
STRUCTURED = list(_STEPS) + ["neg", "one"]


def make_structured(name):
    """fp32 CPU operands of a structured case (the same dict as ``make``)."""
    if name in _STEPS:
        inp = make(*STEP_SHAPE, seed=11)
        j = torch.arange(STEP_SHAPE[1])
        for n in ("q", "k"):
            inp[n] = 0.3 * inp[n]
        inp["q"][..., 0] = 1.0
        inp["k"][..., 0] = _STEPS[name](j).float()
    elif name == "neg":      # every real energy far below zero: a zero taken into the row max underflows every real weight
        inp = make(*NEG_SHAPE, seed=12)
        inp["q"], inp["k"] = inp["q"].abs() + 4.0, -(inp["k"].abs() + 4.0)
        assert torch.bmm(inp["q"], inp["k"].transpose(1, 2)).max().item() < -104.0      # e^-104 < the smallest fp32 denormal
    elif name == "one":      # N = 1: one real key and 63 phantom ones; o = v, lse = the energy, dq = dk = 0
        inp = make(*ONE_SHAPE, seed=13)
    else:
        raise KeyError(name)
    return inp


def conditioning(inp):
    """fp64 scales of the gradients' rounding error: dq = dS K with dS = P (gamma dP - delta), whose rows cancel to zero, so its error
    is relative to |dS|a |K| with |dS|a = P (|gamma dP| + |delta|), not to |dq|; likewise dk; dv = P^T (gamma g) has no cancellation
    beyond the sum's own."""
    q, k, v, g, gamma = (inp[n].double() for n in ("q", "k", "v", "g", "gamma"))
    p = torch.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)
    do = gamma * g
    dp = torch.bmm(do, v.transpose(1, 2))
    delta = (do * torch.bmm(p, v)).sum(dim=-1, keepdim=True)
    dsa = p * (dp.abs() + delta.abs())
    return {"dq": torch.bmm(dsa, k.abs()).max().item(), "dk": torch.bmm(dsa.transpose(1, 2), q.abs()).max().item(),
            "dv": torch.bmm(p.transpose(1, 2), do.abs()).max().item()}


def structured_reference(name):
    """(inputs, fp64 results with ["cond"] = conditioning(inputs)) of a structured case, computed once and shared."""
    key = ("structured", name)
    if key not in _REF:
        inp = make_structured(name)
        ref = evaluate(inp)
        ref["cond"] = conditioning(inp)
        _REF[key] = (inp, ref)
    return _REF[key]


# ---- one measure for every comparison: error / bound, so that > 1 (or a non-finite value) is a miss ------------------------------------
def _rel(a, b):
    a, b = a.detach().double().cpu().reshape(b.shape), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _dgamma_ratio(got, ref):
    return abs(got["dgamma"].detach().double().cpu().reshape(()) - ref["dgamma"].reshape(())).item() / (DGAMMA_ABS * ref["abs_go"].item())


def table_ratios(got, ref):
    """The bounds of the case tables (rel_err's norm: max |err| / max |ref|), each error divided by its bound; keys missing from
    ``got`` are skipped."""
    r = {n: _rel(got[n], ref[n]) / Y_TOL for n in ("y", "o", "lse") if n in got}
    r.update({n: _rel(got[n], ref[n]) / GRAD_TOL for n in ("dq", "dk", "dv", "dx") if n in got})
    if "dgamma" in got:
        r["dgamma"] = _dgamma_ratio(got, ref)
    return r


def structured_ratios(got, ref):
    """The bounds of the structured cases: y, o, lse as the tables; dq, dk, dv by max |err| <= GRAD_TOL * conditioning()."""
    r = {n: _rel(got[n], ref[n]) / Y_TOL for n in ("y", "o", "lse") if n in got}
    for n in ("dq", "dk", "dv"):
        if n in got:
            r[n] = (got[n].detach().double().cpu() - ref[n]).abs().max().item() / (GRAD_TOL * ref["cond"][n])
    if "dgamma" in got:
        r["dgamma"] = _dgamma_ratio(got, ref)
    return r


def misses(ratios, limit=1.0):
    """names whose ratio is past ``limit`` or not finite"""
    return sorted(n for n, v in ratios.items() if not (v <= limit))


# ---- the kernels' ALGORITHM in fp32 on the CPU, with planted faults ---------------------------------------------------------------------
FAULTS = ["phantom_zero", "mask_after_max", "no_alpha", "lse_is_m", "s_drops_tail", "dp_drops_tail", "dchunk1_unwritten",
          "row_pass_stops", "dgamma_first_256", "delta_without_gamma"]


def _contract(a, b, drop_tail):
    """sum over 32-column chunks of a[:, :, chunk] b[:, :, chunk]^T; ``drop_tail`` loses the last chunk if it is a partial one"""
    width = a.shape[2]
    n = width // DK if drop_tail else -(-width // DK)
    out = torch.zeros(a.shape[0], a.shape[1], b.shape[1])
    for ch in range(n):
        out += torch.bmm(a[:, :, DK * ch:DK * (ch + 1)], b[:, :, DK * ch:DK * (ch + 1)].transpose(1, 2))
    return out


def tiled_fp32(inp, fault=None, nt=None):
    """csrc/attention.hip restated step by step in fp32: rows past N staged as zeros, the forward sweep over 64-key tiles with the mask
    before the running max, the rescale by alpha, lse = m + log l; contractions over dq and C in 32-column chunks; the backward's P
    from lse and dS from delta, output columns of dK / dQ per dq chunk; delta and dgamma from a row pass of ``row_blocks`` workers
    that stride over the rows.  ``fault`` plants one of FAULTS."""
    assert fault is None or fault in FAULTS, fault
    q, k, v, x, g = (inp[n].float() for n in ("q", "k", "v", "x", "g"))
    gamma = inp["gamma"].float().reshape(())
    B, N, dq = q.shape
    C = v.shape[2]
    br = branches((B, N, dq, C), nt)
    NP = TILE * br["tiles"]
    pad = lambda t: torch.nn.functional.pad(t, (0, 0, 0, NP - N))      # noqa: E731
    qp, kp, vp, gp = pad(q), pad(k), pad(v), pad(g)
    real = torch.arange(NP) < N
    s_drop = fault == "s_drops_tail"

    # forward: every query row against the key tiles in turn
    m = torch.full((B, NP, 1), float("-inf"))
    l = torch.zeros(B, NP, 1)
    acc = torch.zeros(B, NP, C)
    for y0 in range(0, NP, TILE):
        s = _contract(qp, kp[:, y0:y0 + TILE], s_drop)
        phantom = ~real[y0:y0 + TILE]
        if fault == "mask_after_max":
            mx = s.max(dim=2, keepdim=True).values
            s = s.masked_fill(phantom, float("-inf"))
        else:
            if fault != "phantom_zero":
                s = s.masked_fill(phantom, float("-inf"))
            mx = s.max(dim=2, keepdim=True).values
        mnew = torch.maximum(m, mx)
        alpha = torch.exp(m - mnew)
        p = torch.exp(s - mnew)
        l = l * alpha + p.sum(dim=2, keepdim=True)
        acc = (acc if fault == "no_alpha" else acc * alpha) + torch.bmm(p, vp[:, y0:y0 + TILE])
        m = mnew
    o = (acc * (1.0 / l))[:, :N]
    lse = (m if fault == "lse_is_m" else m + torch.log(l))[:, :N, 0]
    y = gamma * o + x

    # the row pass: worker w takes rows 4 w .. 4 w + 3, then strides by 4 row_blocks
    rb, rows = br["row_blocks"], B * N
    go = (g * o).sum(dim=2).reshape(rows)
    if fault == "row_pass_stops":
        go = torch.where(torch.arange(rows) < 4 * rb, go, torch.zeros(()))      # delta of the rows never reached: left at zero
    delta = ((go if fault == "delta_without_gamma" else gamma * go)).reshape(B, N)
    partial = torch.zeros(rb).index_add_(0, (torch.arange(rows) // 4) % rb, go)
    if fault == "dgamma_first_256":
        dgamma = partial[:256].sum()
    else:
        dgamma = torch.nn.functional.pad(partial, (0, -rb % 256)).reshape(-1, 256).sum(dim=0).sum()

    # backward: P = exp(S - lse), dS = P (gamma dP - delta); swept rows past N contribute nothing
    lse_p = torch.nn.functional.pad(lse, (0, NP - N))
    delta_p = torch.nn.functional.pad(delta, (0, NP - N))
    dp_drop = fault == "dp_drops_tail"
    zero = torch.zeros(())
    dv, dk, d_q = torch.zeros(B, NP, C), torch.zeros(B, NP, dq), torch.zeros(B, NP, dq)
    for y0 in range(0, NP, TILE):
        t = slice(y0, y0 + TILE)
        live = real[t].reshape(1, TILE, 1)
        # keys stationary, queries swept (dV, dK): the statistics belong to the swept row
        p = torch.where(live, torch.exp(_contract(qp[:, t], kp, s_drop) - lse_p[:, t, None]), zero)
        dv += torch.bmm(p.transpose(1, 2), gp[:, t])
        ds = torch.where(live, p * (gamma * _contract(gp[:, t], vp, dp_drop) - delta_p[:, t, None]), zero)
        dk += torch.bmm(ds.transpose(1, 2), qp[:, t])
        # queries stationary, keys swept (dQ): the statistics belong to the lane's own row
        p = torch.exp(_contract(kp[:, t], qp, s_drop) - lse_p[:, None, :])      # a phantom key's is exp(0 - lse): inf where lse < -88
        ds = torch.where(live, p * (gamma * _contract(vp[:, t], gp, dp_drop) - delta_p[:, None, :]), zero)      # a select, as the kernels'
        d_q += torch.bmm(ds.transpose(1, 2), kp[:, t])
    if fault == "dchunk1_unwritten" and br["dchunks"] > 1:
        dk[:, :, 16 * br["nt_d"]:] = 0.0
        d_q[:, :, 16 * br["nt_d"]:] = 0.0
    return {"y": y, "o": o, "lse": lse, "dq": d_q[:, :N], "dk": dk[:, :N], "dv": gamma * dv[:, :N], "dx": g, "dgamma": dgamma.reshape(1)}


# ---- the VP_ATTN_NT child: python -m tests.attention_ref, started by tests/test_gpu_attention.py::test_attn_nt_knob ----------------------
def _knob_child():
    """The fused kernels against fp64 with the channel-chunk knob at 4, at 8 and unset, in a process of its own that sets
    VP_ENV_DYNAMIC before the library loads; prints one JSON line {knob: {case id: {name: error / bound}}, "same_bits": {"knob case id":
    whether every output equals the unset run's bit for bit}}."""
    import json
    import os
    assert os.environ.get("VP_ENV_DYNAMIC") == "1", "the knob is read once per process without VP_ENV_DYNAMIC=1"
    from vae_play_amd import ops
    res, plain = {"same_bits": {}}, {}
    for knob, cases in (("unset", NT_CASES[4] + NT_CASES[8]), ("4", NT_CASES[4]), ("8", NT_CASES[8])):
        if knob == "unset":
            os.environ.pop("VP_ATTN_NT", None)
        else:
            os.environ["VP_ATTN_NT"] = knob
        res[knob] = {}
        for case in cases:
            inp, ref = reference(case)
            t = {n: inp[n].cuda() for n in ("q", "k", "v", "x", "g", "gamma")}
            y, o, lse = ops.attention_fwd(t["q"], t["k"], t["v"], t["x"], t["gamma"])
            d_q, d_k, d_v, dgamma = ops.attention_bwd(t["q"], t["k"], t["v"], o, lse, t["g"], t["gamma"])
            torch.cuda.synchronize()
            got = {n: a.cpu() for n, a in zip(("y", "o", "lse", "dq", "dk", "dv", "dgamma"), (y, o, lse, d_q, d_k, d_v, dgamma))}
            res[knob][case_id(case)] = table_ratios(got, ref)
            if knob == "unset":
                plain[case] = got
            else:      # a column's arithmetic does not depend on the chunk it falls in
                same = all(torch.equal(got[n].view(torch.int32), plain[case][n].view(torch.int32)) for n in got)
                res["same_bits"][knob + " " + case_id(case)] = same
    os.environ.pop("VP_ATTN_NT", None)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    _knob_child()
