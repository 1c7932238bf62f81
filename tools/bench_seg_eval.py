"""Segmentation evaluation: a validation batch of 16 through ``networks_BE.ComposeNet`` at feat 128 x 128 (logit planes
512 x 512) and through the font ``ComposeNet(64)`` (planes 64 x 64), to the per-image sums, terms and counts of both heads on the device, as
  torch    ``segment``, then the same metrics with torch ops on the device (BCE-with-logits, sigmoid, the sums, the comparisons, a
           (2 tol + 1)^2 max-pool for the tolerant match),
  fused    ``evaluate``: the ``predict`` launch list and one vp_seg_eval_f32 call on the plan's logit planes,
at ``tolerance`` 0 and 2, in ONE process on one captured plan, the rows alternated over ``--rounds`` windows; a window is as many calls as
fill ``--window`` seconds and ends in a device synchronise.  The counts of the two routes are asserted equal before anything is timed.
Also timed: ``predict`` alone, and the evaluation launch pair alone with its rate over the heads * n * H * W * 8 bytes it must read.  The
planes it reads were written or read a moment before and fit the 256 MiB Infinity Cache: that rate is a cache-resident one, not HBM's.
Reported per row: the median window's time per call and the spread (min, max); ``fused_faster_by_more_than_spread`` is
max(fused) < min(torch).
usage: python tools/bench_seg_eval.py [--batch 16] [--feat 128x128] [--font 64] [--out profiles/r11_seg_eval.json]
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOLERANCES = (0, 2)


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def calls_for(fn, seconds):
    for _ in range(2):
        fn()
    t = window(fn, 2)
    return max(2, int(seconds / max(t, 1e-6)))


def torch_metrics(x, t, thr, tol, bce_weight=0.5, smooth=1.0):
    """segmentation_metrics' result with torch ops on the device"""
    n = x.shape[0]
    p = torch.sigmoid(x)
    bce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    sums = torch.stack([bce.reshape(n, -1).sum(1), (p * t).reshape(n, -1).sum(1), p.reshape(n, -1).sum(1), t.reshape(n, -1).sum(1)], 1)
    mean_bce = sums[:, 0] / (x.shape[2] * x.shape[3])
    dice = (2 * sums[:, 1] + smooth) / (sums[:, 2] + sums[:, 3] + smooth)
    P, T = x >= thr, t >= 0.5
    if tol:
        k = 2 * tol + 1
        Pd, Td = F.max_pool2d(P.float(), k, 1, tol) > 0, F.max_pool2d(T.float(), k, 1, tol) > 0
    else:
        Pd, Td = P, T
    per = lambda m: m.reshape(n, -1).sum(1)                          # noqa: E731
    counts = torch.stack([per(P), per(T), per(P & T), per(P & Td), per(T & Pd), per(~torch.isfinite(x))], 1).to(torch.int32)
    return {"sums": sums, "terms": torch.stack([mean_bce, dice, bce_weight * mean_bce + 1 - dice], 1), "counts": counts}


def bench_net(name, inf, x, a):
    from vae_play_amd import seg_eval
    n, (H, W) = x.shape[0], inf.logits.shape[3:]
    seg = inf.segment(x)
    # an untrained net's logits sit where they like: the threshold is their median, so that both bits occur; the targets are the
    # thresholded logits moved by one pixel, so the tolerant match has something to find that the plain overlap misses
    thr = float(torch.cat([seg["edges"].flatten(), seg["masks"].flatten()]).median())
    targets = {k: torch.roll(seg[k] >= thr, (1, -1), (2, 3)).float().contiguous() for k in ("edges", "masks")}
    out = {k: v.new_empty((2, n) + v.shape[1:]) for k, v in seg_eval._new_result(n, x.device).items()}
    stacked = torch.stack([targets["edges"], targets["masks"]])
    row = {"net": name, "batch": n, "logits": f"{H}x{W}", "threshold": thr}
    for tol in TOLERANCES:
        ws = seg_eval._workspace(2, n, H, W, tol, x.device)

        def torch_route():
            s = inf.segment(x, threshold=thr)
            return {k: torch_metrics(s[k], targets[k], thr, tol) for k in ("edges", "masks")}

        def fused():
            return inf.evaluate(x, targets["edges"], targets["masks"], threshold=thr, tolerance=tol)

        def predict():
            return inf.predict(x)

        def launch():
            seg_eval._launch(inf.logits.data_ptr(), n * H * W, stacked.data_ptr(), n * H * W, out, 2, n, H, W, thr, 0.5, 0.5, 1.0, tol, ws)

        want, got = torch_route(), fused()
        launch()
        torch.cuda.synchronize()
        for k, head in enumerate(("edges", "masks")):
            assert torch.equal(want[head]["counts"], got[head]["counts"]), (name, tol, head, want[head]["counts"], got[head]["counts"])
            assert torch.equal(out["counts"][k], got[head]["counts"])
            assert torch.allclose(want[head]["terms"], got[head]["terms"], rtol=1e-4, atol=1e-6), (name, tol, head)
        c = got["edges"]["counts"].sum(0).tolist()
        fns = {"torch": torch_route, "fused": fused, "predict": predict, "launch": launch}
        calls = {k: calls_for(f, a.window) for k, f in fns.items()}
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():                # alternated: every round times each row once
                times[k].append(window(f, calls[k]))
        r = {"edge_counts_total": dict(zip(seg_eval.COUNTS, c)), "counts_equal": True}
        for k in fns:
            ms = [t * 1e3 for t in times[k]]
            r[k] = {"ms_per_call": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
                    "calls_per_window": calls[k], "windows": a.rounds}
        moved = 2 * n * H * W * 8
        r["launch"]["bytes_it_must_read"] = moved
        r["launch"]["achieved_GBps_cache_resident"] = round(moved / (r["launch"]["ms_per_call"] * 1e-3) / 1e9, 2)
        r["torch_over_fused"] = round(r["torch"]["ms_per_call"] / r["fused"]["ms_per_call"], 3)
        r["fused_faster_by_more_than_spread"] = r["fused"]["max"] < r["torch"]["min"]
        row[f"tolerance_{tol}"] = r
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--feat", default="128x128")
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--font", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_eval.py measures on the GPU; none is visible")
    import vae_play_amd as V
    from vae_play_amd import networks_BE, networks_BE_font
    h, w = (int(v) for v in a.feat.split("x"))
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(0)
    rows = []
    net = networks_BE.ComposeNet(networks_BE.FeatureNet(None, a.channels, 32)).to("cuda").eval()
    x = torch.randn((a.batch, a.channels, h, w), generator=g).to("cuda").contiguous(memory_format=torch.channels_last)
    inf = V.FusedBEInference(net, a.batch, h, w)
    inf.capture()
    rows.append(bench_net("networks_BE.ComposeNet", inf, x, a))
    del inf, net, x
    net = networks_BE_font.ComposeNet(a.font).to("cuda").eval()
    x = torch.rand((a.batch, 3, a.font, a.font), generator=g).to("cuda")
    inf = V.FusedFontInference(net, a.batch)
    inf.capture()
    rows.append(bench_net(f"networks_BE_font.ComposeNet({a.font})", inf, x, a))
    out = {"metric": "ms per validation batch (both heads: per-image sums, terms and counts on the device)", "unit": "ms",
           "device": torch.cuda.get_device_name(0), "rows": rows,
           "method": "one process, one captured plan per net, rows alternated per round, host clock around a window of calls that ends in a "
                     "device synchronise; median window, spread = min / max over the windows.  The launch row's planes are cache-resident "
                     "(written or read a moment before, within the 256 MiB Infinity Cache): its GB/s is not an HBM rate"}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
