"""Per-layer timings of the eight 4x4 stride-2 layers of the Style-GAN generator (models/network_Style_GAN.py:95-98,101-103,116) at
256 x 256, batch 32, through the C ABI: forward, input gradient and weight gradient in bf16x3 and f32.
usage: python tools/microbench_conv4.py [--out profiles/r06_conv4_bench.json] [--batch 32] [--iters 10] [--reps 7]

  layers   down 32->64 at 256, 64->128 at 128, 128->256 at 64, 256->256 at 32 (Conv2d: forward = gather, input gradient = scatter);
           transposed 256->256 at 16, 256->128 at 32, 128->64 at 64, 64->32 at 128 (forward = scatter + bias, input gradient = gather)
  (a)      the same channel pairs as 3x3 and 5x5 stride-2 layers through the same entry points
  (b)      vp_conv_scatter_bias_* against vp_conv_scatter_* + a torch add, on the transposed layers
  (c)      the weight gradient's tap pairs at 16 taps against single taps (VP_WGRAD_PAIR16=1 | 0, re-read per launch)

Method: device events around windows of --iters launches on preallocated buffers, after a warm-up of every variant of a group; the
variants of a group alternate, --reps repetitions each; median [min, max] in microseconds per launch.  TFLOP/s = 2 M N K / median
with M = B Hs Ws, N = Csmall, K = ks^2 Cbig, computed here."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("VP_ENV_DYNAMIC", "1")      # the library then re-reads its per-launch knobs on every launch (csrc/env.h)

import torch  # noqa: E402

# (name, kind, Cin, Cout, input side)
LAYERS = [("down1", "conv", 32, 64, 256), ("down2", "conv", 64, 128, 128), ("down3", "conv", 128, 256, 64), ("down4", "conv", 256, 256, 32),
          ("up1.convT", "convT", 256, 256, 16), ("up2.convT", "convT", 256, 128, 32), ("up3.convT", "convT", 128, 64, 64),
          ("final.0", "convT", 64, 32, 128)]


def measure(group, iters, reps):
    """group: [(label, fn)]; returns {label: (median, min, max)} in microseconds per launch"""
    for _, fn in group:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _ in group}
    for _ in range(reps):
        for label, fn in group:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            times[label].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {label: (sorted(v)[len(v) // 2], min(v), max(v)) for label, v in times.items()}


class Layer:
    """operands of one layer at kernel size ks: big (B, Cb, Hb, Hb), small (B, Cs, Hs, Hs), weight (Cs, Cb, ks, ks)"""

    def __init__(self, kind, Cin, Cout, side, B, ks):
        from vae_play_amd import _lib, ops
        self.ks = ks
        if kind == "conv":
            self.Cb, self.Cs, self.Hb = Cin, Cout, side
            self.Hs = ops.conv_out_size(side, ks, 2)
        else:
            self.Cb, self.Cs, self.Hs, self.Hb = Cout, Cin, side, 2 * side
            assert ops.conv_out_size(self.Hb, ks, 2) == self.Hs
        self.B = B
        g = torch.Generator(device="cuda").manual_seed(1)
        nhwc = lambda C, H: torch.randn(B, H, H, C, device="cuda", generator=g).permute(0, 3, 1, 2)
        self.big, self.small = nhwc(self.Cb, self.Hb), nhwc(self.Cs, self.Hs)
        self.w = torch.randn(self.Cs, self.Cb, ks, ks, device="cuda", generator=g) * 0.05
        self.bias = torch.randn(self.Cb, device="cuda", generator=g)
        self.out_small, self.out_big = torch.empty_like(self.small), torch.empty_like(self.big)
        self.dw = torch.empty_like(self.w)
        self.p0, self.p1 = ops.pack_w(self.w, True, True)
        self.p0s, self.p1s = ops.pack_w_split(self.w, True, True)
        self.bigs, self.smalls = ops.split_f32(self.big), ops.split_f32(self.small)
        self.geom = (B, self.Hs, self.Hs, self.Hb, self.Hb)
        lib = _lib.load()
        tail = (self.Cb, self.Cs, ks, 2)
        os.environ["VP_WGRAD_PAIR16"] = "1"
        nb = max(lib.vp_conv_wgrad_workspace_bytes(*self.geom, *tail), lib.vp_conv_wgrad_bf16x3_workspace_bytes(*self.geom, *tail))
        os.environ["VP_WGRAD_PAIR16"] = "0"
        nb = max(nb, lib.vp_conv_wgrad_bf16x3_workspace_bytes(*self.geom, *tail))
        os.environ.pop("VP_WGRAD_PAIR16")
        self.ws = ops._ws(nb, self.big)
        self.flops = 2.0 * B * self.Hs * self.Hs * self.Cs * ks * ks * self.Cb

    def calls(self, mode):
        """{family: fn} on the preallocated buffers; family in gather, scatter, scatter_bias, wgrad"""
        from vae_play_amd import _lib, ops
        S, c, P, PV = ops._stream(), _lib.call, ops._p, ops._pv
        g, Cb, Cs, ks = self.geom, self.Cb, self.Cs, self.ks
        nws = self.ws.numel() * 4
        if mode == "f32":
            return {"gather": lambda: c("vp_conv_gather_f32", P(self.big), P(self.p0), None, P(self.out_small), *g, Cb, Cs, ks, 2, 0, S),
                    "scatter": lambda: c("vp_conv_scatter_f32", P(self.small), P(self.p1), P(self.out_big), *g, Cs, Cb, ks, 2, S),
                    "scatter_bias": lambda: c("vp_conv_scatter_bias_f32", P(self.small), P(self.p1), P(self.bias), P(self.out_big), *g, Cs, Cb,
                                              ks, 2, S),
                    "wgrad": lambda: c("vp_conv_wgrad_f32", P(self.big), P(self.small), P(self.dw), *g, Cb, Cs, ks, 2, P(self.ws), nws, S)}
        return {"gather": lambda: c("vp_conv_gather_bf16x3", PV(self.bigs), PV(self.p0s), None, P(self.out_small), *g, Cb, Cs, ks, 2, 0, S),
                "scatter": lambda: c("vp_conv_scatter_bf16x3", PV(self.smalls), PV(self.p1s), P(self.out_big), *g, Cs, Cb, ks, 2, S),
                "scatter_bias": lambda: c("vp_conv_scatter_bias_bf16x3", PV(self.smalls), PV(self.p1s), P(self.bias), P(self.out_big), *g, Cs,
                                          Cb, ks, 2, S),
                "wgrad": lambda: c("vp_conv_wgrad_bf16x3", PV(self.bigs), PV(self.smalls), P(self.dw), *g, Cb, Cs, ks, 2, P(self.ws), nws, S)}


def cell(stat, flops=None):
    med, lo, hi = stat
    d = {"us": round(med, 2), "min_us": round(lo, 2), "max_us": round(hi, 2)}
    if flops is not None:
        d["tflops"] = round(flops / (med * 1e-6) / 1e12, 2)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r06_conv4_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_conv4 needs a GPU: it measures nothing on the CPU")
    from vae_play_amd import _lib
    lib = _lib.load()
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "image": 256, "iters_per_window": a.iters, "repetitions": a.reps,
           "method": "device events around windows of launches on preallocated buffers after warm-up; variants alternate; "
                     "us = median [min, max] per launch; tflops = 2 M N K / median",
           "layers": {}}
    for name, kind, Cin, Cout, side in LAYERS:
        fwd, dgrad = ("gather", "scatter") if kind == "conv" else ("scatter_bias", "gather")
        entry = {"kind": kind, "Cin": Cin, "Cout": Cout, "input_side": side}
        for mode in ("bf16x3", "f32"):
            m = entry[mode] = {}
            # the layer itself and (a) its 3x3 and 5x5 forms: the three kernel sizes alternate per family
            layers = {ks: Layer(kind, Cin, Cout, side, a.batch, ks) for ks in (4, 3, 5)}
            for role, fam in (("forward", fwd), ("input_grad", dgrad), ("weight_grad", "wgrad")):
                st = measure([(ks, L.calls(mode)[fam]) for ks, L in layers.items()], a.iters, a.reps)
                m[role] = dict(cell(st[4], layers[4].flops), family=fam)
                m.setdefault("as_3x3", {})[role] = cell(st[3], layers[3].flops)
                m.setdefault("as_5x5", {})[role] = cell(st[5], layers[5].flops)
            L = layers[4]
            del layers
            calls = L.calls(mode)
            if kind == "convT":      # (b) the fused bias against scatter + a torch add over the full-size output
                bias4 = L.bias.view(1, -1, 1, 1)

                def composed():
                    calls["scatter"]()
                    L.out_big.add_(bias4)
                st = measure([("fused", calls["scatter_bias"]), ("composed", composed)], a.iters, a.reps)
                m["bias_fused_vs_composed"] = {"fused": cell(st["fused"]), "scatter_plus_torch_add": cell(st["composed"])}
            if mode == "bf16x3":     # (c) tap pairs at 16 taps: only where the knob changes the launch
                def with_knob(v):
                    def fn():
                        os.environ["VP_WGRAD_PAIR16"] = v
                        calls["wgrad"]()
                    return fn
                os.environ["VP_WGRAD_PAIR16"] = "0"
                single = lib.vp_conv_wgrad_bf16x3_workspace_bytes(*L.geom, L.Cb, L.Cs, 4, 2)
                os.environ["VP_WGRAD_PAIR16"] = "1"
                pairs = lib.vp_conv_wgrad_bf16x3_workspace_bytes(*L.geom, L.Cb, L.Cs, 4, 2)
                if L.Cb in (32, 64) and L.Cs % 64 == 0:
                    st = measure([("pairs", with_knob("1")), ("single", with_knob("0"))], a.iters, a.reps)
                    m["wgrad_tap_pairs_nt16"] = {"pairs": cell(st["pairs"], L.flops), "single_taps": cell(st["single"], L.flops),
                                                 "workspace_bytes": {"pairs": pairs, "single_taps": single}}
                os.environ.pop("VP_WGRAD_PAIR16")
            del L, calls
            torch.cuda.empty_cache()
        res["layers"][name] = entry
        print(name, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
