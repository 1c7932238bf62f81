#!/usr/bin/env python
"""SelfAttentionBlock core micro-benchmark: the flash-style kernels ("fused") against the per-image GEMM route ("gemm", the code
path the block ran on before, kept in-tree behind ``set_attention_route``), in ONE process.

Shapes (B, C, N) with dq = C // 8, as the reference's users of the block run it: (16, 256, 258) networks_BC.RefineNet,
(4, 720, 2048) networks_BP.ValueEncoder / EmitLineParamPredictor, and the small (2, 32, 16).  q and k are ReLU'd normals (the
block's projections end in a ReLU), v, x and the upstream gradient are normals, gamma = 0.7.  For C > 64 the fused route is timed
with both channel-chunk widths of the forward / dV kernels (128, the plan's choice, and 64).

Per shape: the routes' outputs and gradients are first ASSERTED equal within the bounds of tests/test_gpu_attention.py; then forward
(under no_grad) and forward + backward (through autograd) are timed.  Each figure is the median over ``--reps`` windows of
``--iters`` calls, a window bracketed by device events on the launch stream (host gaps between launches are inside it: the GEMM route
is launch-bound at small N and that is part of what it costs); the variants alternate inside every repetition and min / max over the
repetitions are the spread.  Also recorded: entry-point calls (counted with _lib.TRACE in an untimed run), the peak of
torch.cuda.max_memory_allocated() over one forward + backward above the inputs, and for the fused route the achieved fp32-MFMA rate
against the 157 TF/s roof.  That rate counts every product the kernels perform on the N x N real pairs, the RECOMPUTED ones
included (S once per channel chunk forward and in dV, S and dP in both dK and dQ); padding to the 64-row tiles is not counted.

    python tools/bench_attention.py --out profiles/r12_attention.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("VP_ENV_DYNAMIC", "1")      # lets one process alternate VP_ATTN_NT (the channel-chunk A/B switch)

import torch  # noqa: E402

SHAPES = ((16, 256, 258), (4, 720, 2048), (2, 32, 16))      # (B, C, N)
# --sweep: between the two reference shapes, to place the boundary of the "auto" route (functional.attention_route_for)
SWEEP = ((16, 256, 512), (16, 256, 1024), (4, 256, 2048), (4, 720, 512), (4, 720, 1024), (1, 720, 2048))
MFMA_F32_ROOF_TF = 157.0
Y_TOL, GRAD_TOL = 2e-5, 5e-5


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def ab(variants, iters, reps, warmup):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(window(fn, iters))
    return {k: {"ms": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()}


def fused_flops(B, N, dq, C, chunk):
    """(forward, backward) products the fused kernels perform on real pairs, recomputation included."""
    nch = -(-C // chunk)
    pairs = B * N * N
    fwd = pairs * (2 * dq * nch + 2 * C)
    dv = pairs * (2 * dq * nch + 2 * C)
    dk = pairs * (2 * dq + 2 * C + 2 * dq)
    return fwd, dv + 2 * dk


def rel_err(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()


def bench_shape(B, C, N, args):
    import vae_play_amd
    from vae_play_amd import _lib, functional as F_hip
    dq = max(1, C // 8)
    gen = torch.Generator().manual_seed(0)
    mk = lambda c, relu=False: (torch.relu(torch.randn(B, N, c, generator=gen)) if relu else torch.randn(B, N, c, generator=gen)).cuda()  # noqa: E731
    to4 = lambda t: t.view(B, N, 1, t.shape[2]).permute(0, 3, 1, 2)      # noqa: E731  the channels_last (B, c, N, 1) view of the same memory
    q, k, v, x, g = (to4(t) for t in (mk(dq, True), mk(dq, True), mk(C), mk(C), mk(C)))
    gamma = torch.full((1,), 0.7, device="cuda")
    leaves = [t.detach().requires_grad_(True) for t in (x, q, k, v, gamma)]
    frozen = [t.detach() for t in (x, q, k, v, gamma)]

    def variant(route, nt=None):
        def setup():
            vae_play_amd.set_attention_route(route)
            if nt is None:
                os.environ.pop("VP_ATTN_NT", None)
            else:
                os.environ["VP_ATTN_NT"] = str(nt)

        def fwd():
            setup()
            with torch.no_grad():
                return F_hip.self_attention(*frozen)

        def fwd_bwd():
            setup()
            y = F_hip.self_attention(*leaves)
            return (y,) + torch.autograd.grad(y, leaves, g)
        return fwd, fwd_bwd

    names = {"fused": ("fused", None), "gemm": ("gemm", None)}
    if C > 64:
        names["fused_chunk64"] = ("fused", 4)
    fns = {n: variant(*a) for n, a in names.items()}

    # same function first, asserted; then calls and peak memory in untimed runs
    ref = fns["gemm"][1]()
    agree = {}
    for n in names:
        if n == "gemm":
            continue
        out = fns[n][1]()
        errs = [rel_err(a, b) for a, b in zip(out[:5], ref[:5])]      # y, dx, dq, dk, dv
        assert errs[0] <= Y_TOL and max(errs[1:]) <= GRAD_TOL, (n, errs)
        agree[n] = dict(zip(("y", "dx", "dq", "dk", "dv"), errs))
        agree[n]["dgamma_abs"] = abs(out[5].item() - ref[5].item())
    res = {"shape": {"B": B, "C": C, "N": N, "dq": dq}, "max_rel_diff_vs_gemm": agree, "forward": {}, "forward_backward": {}}
    for n in names:
        for mode, idx in (("forward", 0), ("forward_backward", 1)):
            _lib.TRACE = {"events": []}
            fns[n][idx]()
            torch.cuda.synchronize()
            res[mode].setdefault(n, {})["entry_point_calls"] = len(_lib.TRACE["events"])
            _lib.TRACE = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fns[n][1]()
        torch.cuda.synchronize()
        res["forward_backward"][n]["peak_bytes_above_inputs"] = torch.cuda.max_memory_allocated() - base
        del out
    del ref
    for mode, idx in (("forward", 0), ("forward_backward", 1)):
        r = ab({n: fns[n][idx] for n in names}, args.iters, args.reps, args.warmup)
        for n in names:
            res[mode][n].update(r[n])
            if n != "gemm":
                f, b = fused_flops(B, N, dq, C, 64 if n == "fused_chunk64" or C <= 64 else 128)
                flops = f if idx == 0 else f + b
                res[mode][n]["mfma_flops_recompute_included"] = flops
                res[mode][n]["TF_per_s"] = flops / (r[n]["ms"] * 1e-3) / 1e12
                res[mode][n]["share_of_f32_mfma_roof"] = res[mode][n]["TF_per_s"] / MFMA_F32_ROOF_TF
        m = res[mode]
        m["speedup_fused_vs_gemm"] = m["gemm"]["ms"] / m["fused"]["ms"]
        m["fused_faster_beyond_spread"] = bool(m["fused"]["max"] < m["gemm"]["min"])
        m["gemm_faster_beyond_spread"] = bool(m["gemm"]["max"] < m["fused"]["min"])
        print(f"B{B} C{C} N{N} {mode}: " + "  ".join(
            f"{n} {m[n]['ms']:.3f} ms [{m[n]['min']:.3f}, {m[n]['max']:.3f}] {m[n]['entry_point_calls']} calls"
            + (f" {m[n]['TF_per_s']:.1f} TF/s" if n != "gemm" else "") for n in names) + f"  x{m['speedup_fused_vs_gemm']:.2f}", flush=True)
    vae_play_amd.set_attention_route("auto")
    os.environ.pop("VP_ATTN_NT", None)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=7, help="windows per variant (alternating)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", action="store_true", help="also time the shapes of SWEEP (recorded under 'sweep')")
    ap.add_argument("--out", default="profiles/r12_attention.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention.py measures on the GPU; none is visible")
    doc = {"tool": "tools/bench_attention.py", "device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps,
           "f32_mfma_roof_TF_per_s": MFMA_F32_ROOF_TF,
           "timing": "device events around a window of calls (host gaps included); median [min, max] over alternating repetitions",
           "flops": "fused route only: products on the B N N real pairs, recomputed ones included (S per channel chunk in forward and dV; "
                    "S and dP in both dK and dQ); tile padding not counted",
           "results": {}}
    for B, C, N in SHAPES:
        doc["results"][f"B{B}_C{C}_N{N}"] = bench_shape(B, C, N, args)
    if args.sweep:
        doc["sweep"] = {f"B{B}_C{C}_N{N}": bench_shape(B, C, N, args) for B, C, N in SWEEP}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
