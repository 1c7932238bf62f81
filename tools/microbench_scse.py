#!/usr/bin/env python
"""SCSEBlock micro-benchmark: the fused HIP block against the same block composed from the library's other ops, in ONE process.

At the three StyleUp stage tensors of the Style-GAN generator (256x256 images, batch 32, NHWC fp32: 32x32x32x256, 32x64x64x128,
32x128x128x64; reduction 4), forward only and forward + backward:
  fused      -- functional.scse (what blocks.SCSEBlock.forward calls), through autograd
  fused_abi  -- the same kernels called at the C ABI on preallocated buffers (no autograd, no allocation: the kernels' own time)
  composed   -- global_avg_pool + three 1x1 conv2d of this library + torch sigmoid / relu / mul / add, through autograd.  Built
                here for the comparison only; it is not a product path.
Each figure is the median over ``--reps`` windows of ``--iters`` calls, a window bracketed by device events on the launch stream
(host gaps between launches are inside it); the variants alternate inside every repetition and min / max over the repetitions are
the spread.  Every variant is warmed up first.  Bytes are what the fused schedule must move: 3 passes over the tensor forward
(two reads of x, one write of y), 5 backward (x, dy, dx written, dx read and written once more), against the ~6.3 TB/s a
streaming copy reaches on the MI355X.

    python tools/microbench_scse.py --out profiles/r05_scse_bench.json
"""
import argparse
import json
import os
import statistics
import sys
from ctypes import c_void_p

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = ((32, 256, 32, 32), (32, 128, 64, 64), (32, 64, 128, 128))      # (B, C, H, W)
REDUCTION = 4
HBM_COPY_TBS = 6.3


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


def composed(x, w1, b1, w2, b2, ws, bs):
    from vae_play_amd import functional as F_hip
    B, C = x.shape[:2]
    pooled = F_hip.global_avg_pool(x).reshape(B, C, 1, 1)
    c = torch.sigmoid(F_hip.conv2d(torch.relu(F_hip.conv2d(pooled, w1, b1)), w2, b2))
    s = torch.sigmoid(F_hip.conv2d(x, ws, bs))
    return x * c + x * s


def bench_shape(B, C, H, W, args):
    from vae_play_amd import _lib, functional as F_hip
    from vae_play_amd.blocks import SCSEBlock
    lib = _lib.load()
    torch.manual_seed(0)
    blk = SCSEBlock(C, reduction=REDUCTION).cuda()
    p = [blk.cSE[1].weight, blk.cSE[1].bias, blk.cSE[3].weight, blk.cSE[3].bias, blk.sSE[0].weight, blk.sSE[0].bias]
    x = torch.randn(B, C, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    dy = torch.randn(B, C, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    xg = x.clone().requires_grad_(True)
    n, hid, HW = x.numel(), C // REDUCTION, H * W

    # the C ABI on preallocated buffers
    P = lambda a: c_void_p(a.data_ptr())      # noqa: E731
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    new = lambda *s: torch.empty(*s, device="cuda")      # noqa: E731
    y, dx = torch.empty_like(x), torch.empty_like(x)
    pool, hidden, cg, sg = new(B, C), new(B, hid), new(B, C), new(B, HW)
    g = [torch.empty_like(q) for q in p]
    nbytes = lib.vp_scse_workspace_bytes(B, HW, C, hid)
    wk = new(nbytes // 4 + 4)
    pd = [q.detach() for q in p]

    def abi_fwd():
        _lib.check(lib.vp_scse_fwd_f32(P(x), *(P(q) for q in pd), P(y), P(pool), P(hidden), P(cg), P(sg), B, HW, C, hid, 0, P(wk), nbytes, st))

    def abi_fwd_bwd():
        abi_fwd()
        _lib.check(lib.vp_scse_bwd_f32(P(x), P(dy), P(pd[0]), P(pd[2]), P(pd[4]), P(pool), P(hidden), P(cg), P(sg), P(dx),
                                       *(P(q) for q in g), B, HW, C, hid, 0, P(wk), nbytes, st))

    def fused_fwd():
        with torch.no_grad():
            F_hip.scse(x, *p)

    def composed_fwd():
        with torch.no_grad():
            composed(x, *p)

    def fused_fwd_bwd():
        torch.autograd.grad(F_hip.scse(xg, *p), [xg] + p, dy)

    def composed_fwd_bwd():
        torch.autograd.grad(composed(xg, *p), [xg] + p, dy)

    # same function first (recorded, not asserted: tests/test_gpu_scse.py asserts against fp64)
    with torch.no_grad():
        diff = (F_hip.scse(x, *p) - composed(x, *p)).abs().max().item()
    out = {"shape_BCHW": [B, C, H, W], "tensor_MB": n * 4 / 1e6, "max_abs_diff_fused_vs_composed_y": diff}
    for mode, variants, passes in (("forward", {"fused": fused_fwd, "fused_abi": abi_fwd, "composed": composed_fwd}, 3),
                                   ("forward_backward", {"fused": fused_fwd_bwd, "fused_abi": abi_fwd_bwd, "composed": composed_fwd_bwd}, 8)):
        r = ab(variants, args.iters, args.reps, args.warmup)
        moved = passes * n * 4
        r["fused_bytes_moved"] = moved
        for k in ("fused", "fused_abi"):
            r[k]["TB_per_s"] = moved / (r[k]["ms"] * 1e-3) / 1e12
            r[k]["share_of_streaming_copy"] = r[k]["TB_per_s"] / HBM_COPY_TBS
        r["speedup_fused_vs_composed"] = r["composed"]["ms"] / r["fused"]["ms"]
        # faster by more than the spread: the slowest fused window is still below the fastest composed window
        r["fused_faster_beyond_spread"] = bool(r["fused"]["max"] < r["composed"]["min"])
        out[mode] = r
        print(f"{B}x{H}x{W}x{C} {mode}: fused {r['fused']['ms']:.3f} ms [{r['fused']['min']:.3f}, {r['fused']['max']:.3f}] "
              f"({r['fused']['TB_per_s']:.2f} TB/s)  abi {r['fused_abi']['ms']:.3f} [{r['fused_abi']['min']:.3f}, {r['fused_abi']['max']:.3f}] "
              f"({r['fused_abi']['TB_per_s']:.2f} TB/s)  composed {r['composed']['ms']:.3f} [{r['composed']['min']:.3f}, "
              f"{r['composed']['max']:.3f}]  x{r['speedup_fused_vs_composed']:.2f}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=7, help="windows per variant (alternating)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="profiles/r05_scse_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_scse.py measures on the GPU; none is visible")
    doc = {"tool": "tools/microbench_scse.py", "device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps,
           "reduction": REDUCTION, "streaming_copy_TB_per_s": HBM_COPY_TBS,
           "timing": "device events around a window of calls (host gaps included); median [min, max] over alternating repetitions",
           "bytes": "fused schedule: 3 passes over the tensor forward, 5 backward (partials and gates are < 3 % more)",
           "results": {}}
    for B, C, H, W in SHAPES:
        doc["results"][f"{B}x{H}x{W}x{C}"] = bench_shape(B, C, H, W, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
