"""Font U-Net inference (test_BE_font.py:99): ``networks_BE_font.ComposeNet(in_size)`` on a batch of glyph images with ``y=None``, as
  modules  the drop-in modules in ``.eval()`` under ``torch.no_grad()`` (the autograd front end, one launch per module piece),
  eager    ``FusedFontInference.predict`` running its launch list,
  graph    the same after ``capture()`` (one hipGraph replay),
in ONE process, the three rows alternated over ``--rounds`` windows each; a window is as many calls as fill ``--window`` seconds and
ends in a device synchronise.  Reported per row: the median window's time per call and the spread (min, max) over the windows.  All
rows get the same channels_last input and return the two logit maps; the fused rows include ``predict``'s copy of the input into the
plan's buffer and of the logits out of it.
usage: python tools/bench_font_infer.py [--sizes 64,256] [--batch 16] [--precisions f32,bf16x3] [--out profiles/r08_font_infer.json]
       python tools/bench_font_infer.py --layers [--sizes 64] [--out profiles/r08_font_infer_layers.json]
Prints one JSON line (and writes it to --out).  ``--layers`` times no rows: for every InstanceNorm layer of the f32 plan whose shape
the whole-image convolution + InstanceNorm kernel takes (``vp_conv_in_supported``; whether the plan runs it there is
``plan_uses_kernel`` = ``vp_conv_in_preferred``) it times that launch next to the pair it replaces (the existing convolution entry and
the InstanceNorm entry, on the same input and weights), each as a device event pair around ``--reps`` back-to-back calls, the two
alternated over ``--rounds`` rounds; median and spread."""
import argparse
import json
import os
import statistics
import sys
import time
from ctypes import c_void_p

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


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def layer_times(inf, x, reps, rounds):
    """every vp_conv_in_act_f32 launch of the plan next to vp_conv_gather_f32 + vp_instnorm_act_fwd_f32 on the same operands"""
    from vae_play_amd import _lib
    lib = _lib.load()
    inf.predict(x)                                   # every layer's input buffer holds real activations
    torch.cuda.synchronize()
    s = c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: c_void_p(t.data_ptr())             # noqa: E731
    rows, seen = [], {}
    for plan in inf._plans["predict.cl"]:
        for ci, (name, fn, args, slot, flops, tag, _, _) in enumerate(plan.calls):
            if name == "vp_conv_in_act_f32":
                xin, wp, _, _, B, H, W, cin, cout, ks, stride, eps, act, slope = args[:14]
            elif name == "vp_conv_gather_f32" and plan.calls[ci + 1][0].startswith("vp_instnorm_act_fwd"):
                # a layer the plan keeps on the pair: time the kernel on it too where it takes the shape
                xin, wp, _, _, B, _, _, H, W, cin, cout, ks, stride = args[:13]
                nxt = plan.calls[ci + 1]
                eps, act, slope = nxt[2][8:11] if nxt[0].endswith("_ld_f32") else nxt[2][7:10]
                if not lib.vp_conv_in_supported(H, W, cin, cout, ks, stride):
                    continue
            else:
                continue
            key = (B, H, W, cin, cout, ks, stride)
            if key in seen:
                seen[key]["layers"].append(tag[:-4])
                continue
            pad = (ks - 1) // 2
            Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
            R = Ho * Wo
            y1, y2, c = (torch.empty((B, R, cout), device="cuda") for _ in range(3))
            mean, rstd = torch.empty((B, cout), device="cuda"), torch.empty((B, cout), device="cuda")
            nws = lib.vp_instnorm_workspace_bytes(B, R, cout)
            ws = torch.empty(max(1, (nws + 3) // 4), device="cuda")

            def fused():
                _lib.check(lib.vp_conv_in_act_f32(xin, wp, P(y1), cout, B, H, W, cin, cout, ks, stride, eps, act, slope, s), "fused")

            def pair():     # (the packed weight has vp_pack_w_f32's layout: [Cout][ks*ks][Cin])
                _lib.check(lib.vp_conv_gather_f32(xin, wp, None, P(c), B, Ho, Wo, H, W, cin, cout, ks, stride, 0, s), "conv")
                _lib.check(lib.vp_instnorm_act_fwd_f32(P(c), P(y2), P(mean), P(rstd), B, R, cout, eps, act, slope, P(ws), nws, s), "instnorm")
            for _ in range(3):
                fused()
                pair()
            torch.cuda.synchronize()
            diff = float((y1 - y2).abs().max() / y2.abs().max().clamp_min(1e-30))
            tf, tp = [], []
            for _ in range(rounds):
                tf.append(event_ms(fused, reps))
                tp.append(event_ms(pair, reps))
            row = {"layers": [tag[:-4]], "B": B, "in": f"{H}x{W}", "out": f"{Ho}x{Wo}", "cin": cin, "cout": cout, "ks": ks, "stride": stride,
                   "fused_us": round(statistics.median(tf) * 1e3, 2), "fused_min_max_us": [round(min(tf) * 1e3, 2), round(max(tf) * 1e3, 2)],
                   "pair_us": round(statistics.median(tp) * 1e3, 2), "pair_min_max_us": [round(min(tp) * 1e3, 2), round(max(tp) * 1e3, 2)],
                   "max_rel_diff": diff}
            row["pair_over_fused"] = round(row["pair_us"] / row["fused_us"], 3)
            row["plan_uses_kernel"] = bool(lib.vp_conv_in_preferred(H, W, cin, cout, ks, stride))
            seen[key] = row
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256", help="in_size of ComposeNet (64: test_BE_font.py's default)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--precisions", default="f32,bf16x3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of work per timed window")
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--reps", type=int, default=50, help="--layers: back-to-back calls inside one event pair")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_font_infer.py measures on the GPU; none is visible")
    import vae_play_amd as V
    from vae_play_amd import networks_BE_font
    rows_out = []
    for S in (int(v) for v in a.sizes.split(",")):
        torch.manual_seed(0)
        net = networks_BE_font.ComposeNet(S).to("cuda").eval()
        x = torch.rand((a.batch, 3, S, S), generator=torch.Generator().manual_seed(1)).to("cuda")
        x = x.contiguous(memory_format=torch.channels_last)
        if a.layers:
            eager = V.FusedFontInference(net, a.batch, precision="f32")
            rows_out.append({"net": f"ComposeNet({S})", "batch": a.batch, "layers": layer_times(eager, x, a.reps, a.rounds)})
            del eager, net
            continue
        for prec in a.precisions.split(","):
            eager = V.FusedFontInference(net, a.batch, precision=prec)
            graph = V.FusedFontInference(net, a.batch, precision=prec)
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
            row = {"net": f"ComposeNet({S})", "input": f"{a.batch}x3x{S}x{S}", "precision": prec,
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
        del net
    out = {"metric": "ms per call (networks_BE_font.ComposeNet inference, y=None, both heads' logits)", "unit": "ms",
           "device": torch.cuda.get_device_name(0), "rows": rows_out,
           "method": "one process, rows alternated per round, host clock around a window of calls that ends in a device synchronise; "
                     "median window, spread = min / max over the windows"}
    if a.layers:
        out["metric"] = "us per launch: the whole-image convolution + InstanceNorm kernel next to the convolution + InstanceNorm pair it replaces"
        out["method"] = f"a device event pair around {a.reps} back-to-back calls, the two alternated over {a.rounds} rounds; median, min / max"
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
