"""Segmentation inference below the backbone (test_BE.py:92-98): ``networks_BE.ComposeNet`` on a 256-channel stride-4 feature map, as
  modules  the drop-in modules in ``.eval()`` under ``torch.no_grad()`` (the autograd front end, one launch per module piece),
  eager    ``FusedBEInference.predict`` running its launch list,
  graph    the same after ``capture()`` (one hipGraph replay),
in ONE process, the three rows alternated over ``--rounds`` windows each; a window is as many calls as fill ``--window`` seconds and
ends in a device synchronise.  Reported per row: the median window's time per call and the spread (min, max) over the windows.  All
rows get the same channels_last input and return the two logit maps; the fused rows include ``predict``'s copy of the input into the
plan's buffer and of the logits out of it.
usage: python tools/bench_be_infer.py [--shapes 64x64,128x128] [--batch 16] [--precisions f32,bf16x3] [--out profiles/r07_be_infer.json]
       python tools/bench_be_infer.py --launches-only [--out profiles/r07_be_infer_launches.json]
Prints one JSON line (and writes it to --out).  ``--launches-only`` times no rows: it brackets every launch of the eager list with
a device event pair (``_Plan.run``'s timers) and reports the mean over 20 runs per launch -- where the fused list's time goes."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def calls_for(fn, seconds):
    for _ in range(3):
        fn()
    t = window(fn, 3)
    return max(5, int(seconds / max(t, 1e-6)))


def module_launches(fn):
    """entry points the module path goes through in one call (vae_play_amd._lib.call's trace)"""
    from vae_play_amd import _lib
    _lib.TRACE = {"events": []}
    try:
        fn()
        torch.cuda.synchronize()
        return len(_lib.TRACE["events"])
    finally:
        _lib.TRACE = None


def launch_times(inf, x, reps=20):
    """mean device time of each launch of the eager predict list, from event pairs around the launches"""
    src, cl, static = inf._feed(x)
    inf._load(static, src)
    plans = inf._plans["predict" + cl]
    names = {c[0] for p in plans for c in p.calls}
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        for p in plans:
            p.run(s)
    total = {}
    for _ in range(reps):
        tm = {"names": names, "events": []}
        for p in plans:
            p.run(s, timers=tm)
        torch.cuda.synchronize()
        for i, (name, tag, _, e0, e1) in enumerate(tm["events"]):
            total[(i, name, tag)] = total.get((i, name, tag), 0.0) + e0.elapsed_time(e1)
    return [{"launch": name, "tag": tag, "ms": round(v / reps, 4)} for (_, name, tag), v in sorted(total.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x64,128x128", help="feature-map sizes (64x64: tools/bench_be_heads.py's; 128x128: test_BE.py's "
                    "default --img_size 512)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--precisions", default="f32,bf16x3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of work per timed window")
    ap.add_argument("--launches-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_be_infer.py measures on the GPU; none is visible")
    import vae_play_amd as V
    from vae_play_amd import networks_BE
    torch.manual_seed(0)
    net = networks_BE.ComposeNet(networks_BE.FeatureNet(None, a.channels, 32)).to("cuda").eval()
    rows_out = []
    for shape in a.shapes.split(","):
        h, w = (int(v) for v in shape.split("x"))
        x = torch.randn((a.batch, a.channels, h, w), generator=torch.Generator().manual_seed(1)).to("cuda")
        x = x.contiguous(memory_format=torch.channels_last)
        for prec in a.precisions.split(","):
            eager = V.FusedBEInference(net, a.batch, h, w, precision=prec)
            if a.launches_only:
                per = launch_times(eager, x)
                rows_out.append({"feature": f"{a.batch}x{a.channels}x{h}x{w}", "precision": prec, "launches": per,
                                 "sum_ms": round(sum(r["ms"] for r in per), 4)})
                continue
            graph = V.FusedBEInference(net, a.batch, h, w, precision=prec)
            graph.capture()

            def modules():
                V.set_conv_precision(prec)
                try:
                    with torch.no_grad():
                        return net(x)
                finally:
                    V.set_conv_precision("f32")
            fns = {"modules": modules, "eager": lambda: eager.predict(x), "graph": lambda: graph.predict(x)}
            ref = modules()
            err = {k: max(float((fns[k]()[m] - ref[m]).abs().max() / ref[m].abs().max()) for m in ("edges", "masks")) for k in ("eager", "graph")}
            n = {k: calls_for(f, a.window) for k, f in fns.items()}
            times = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, f in fns.items():        # alternated: every round times each row once
                    times[k].append(window(f, n[k]))
            row = {"feature": f"{a.batch}x{a.channels}x{h}x{w}", "precision": prec,
                   "fused_launches": len([c for p in eager._plans["predict.cl"] for c in p.calls]),
                   "module_launches": module_launches(modules), "max_rel_diff_vs_modules": err}
            for k in fns:
                ms = [t * 1e3 for t in times[k]]
                row[k] = {"ms_per_call": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
                          "calls_per_window": n[k], "windows": a.rounds}
            row["modules_over_eager"] = round(row["modules"]["ms_per_call"] / row["eager"]["ms_per_call"], 3)
            row["modules_over_graph"] = round(row["modules"]["ms_per_call"] / row["graph"]["ms_per_call"], 3)
            rows_out.append(row)
            del eager, graph
    out = {"metric": "ms per call (networks_BE.ComposeNet inference below the backbone, both heads' logits)", "unit": "ms",
           "device": torch.cuda.get_device_name(0), "rows": rows_out,
           "method": "one process, rows alternated per round, host clock around a window of calls that ends in a device synchronise; "
                     "median window, spread = min / max over the windows"}
    if a.launches_only:
        out["metric"], out["method"] = "ms per launch of the fused eager predict list", "a device event pair around each launch, mean of 20 runs"
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
