"""The label-gated convolution pairs of the Style-GAN generator (models/network_Style_GAN.py:72-79,92-98), fused against composed:
network_Style_GAN._PAIR_FUSED on (one stacked convolution + functional.pair_blend) against off (the reference's expression over two
Conv2d blocks), forward + backward through the autograd front end, in bf16x3 and f32.
usage: python tools/microbench_pairconv.py [--out profiles/r07_pairconv_bench.json] [--batch 32] [--iters 5] [--reps 7] [--no-generator]

  (a) layers     conv1 4->32 and conv2 32->32 (3x3, stride 1, bn=None, no activation) at 256; down1 32->64 at 256, down2 64->128 at 128,
                 down3 128->256 at 64, down4 256->256 at 32 (4x4, stride 2, InstanceNorm + ReLU): the whole layer, and its
                 normalise-and-blend part alone on a given convolution output (fused: pair_blend of u (B, 2C, H, W); composed: two
                 instance_norm_act / nothing, then torch's mul, mul, add on u1, u2 (B, C, H, W))
  (b) generator  one Generator(256, 512) forward + backward both ways (the only place its 1.5 GB mlp layer is instantiated)

Method: one process; device events around windows of --iters forward + backward passes after a warm-up of both variants; the variants
alternate, --reps repetitions each; median [min, max] in microseconds per forward + backward.  In bf16x3 mode a layer's input carries
its split planes, as the output of the layer before it does in the network."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

# (name, Cin, Cout, kernel, stride, bn, activate, input side at image size 256)
LAYERS = [("conv1", 4, 32, 3, 1, None, None, 256), ("conv2", 32, 32, 3, 1, None, None, 256), ("down1", 32, 64, 4, 2, "instance", "relu", 256),
          ("down2", 64, 128, 4, 2, "instance", "relu", 128), ("down3", 128, 256, 4, 2, "instance", "relu", 64),
          ("down4", 256, 256, 4, 2, "instance", "relu", 32)]


def measure(group, iters, reps):
    """group: [(label, fn)]; returns {label: (median, min, max)} in microseconds per call"""
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


def cell(stat):
    med, lo, hi = stat
    return {"us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1)}


def verdict(fused, composed):
    """section 16(b)'s rule: the fused form wins only where its median is below the composed one's beyond the [min, max] spread"""
    if fused[2] < composed[1]:
        return "fused"
    if composed[2] < fused[1]:
        return "composed"
    return "inside the spread"


def nhwc(B, C, H, gen):
    return torch.randn(B, H, H, C, device="cuda", generator=gen).permute(0, 3, 1, 2)


def layer_rows(name, Cin, Cout, ks, stride, bn, act, side, B, mode, iters, reps):
    from vae_play_amd import functional as FH, network_Style_GAN as N, ops
    gen = torch.Generator(device="cuda").manual_seed(1)
    torch.manual_seed(0)
    mod = N.myConv2d(Cin, Cout, ks, stride, bn, act).cuda()
    x = nhwc(B, Cin, side, gen).requires_grad_(True)
    if mode == "bf16x3" and Cin % 8 == 0:
        x._vp_split = (ops.split_f32(x.detach()), x._version)
    out = ops.conv_out_size(side, ks, stride)
    gy = nhwc(B, Cout, out, gen)
    label = (torch.arange(B, device="cuda") % 2).reshape(B, 1, 1, 1)         # int64 0 / 1, as train_Style_GAN.py passes it

    def whole(fused):
        def fn():
            N._PAIR_FUSED = fused
            mod.zero_grad(set_to_none=True)
            x.grad = None
            mod(x, label).backward(gy)
        return fn

    st = measure([("fused", whole(True)), ("composed", whole(False))], iters, reps)
    row = {"layer": {"fused": cell(st["fused"]), "composed": cell(st["composed"]), "faster": verdict(st["fused"], st["composed"])}}
    # the normalise-and-blend part alone, on given convolution outputs
    u = nhwc(B, 2 * Cout, out, gen).requires_grad_(True)
    u1, u2 = nhwc(B, Cout, out, gen).requires_grad_(True), nhwc(B, Cout, out, gen).requires_grad_(True)
    labf = label.float()

    def blend_fused():
        u.grad = None
        FH.pair_blend(u, label, bn == "instance", 1e-5, act).backward(gy)

    def blend_composed():
        u1.grad = u2.grad = None
        a1, a2 = (FH.instance_norm_act(v, 1e-5, act) if bn == "instance" else FH.activation(v, act) for v in (u1, u2))
        (a1 * (1 - labf) + a2 * labf).backward(gy)

    st = measure([("fused", blend_fused), ("composed", blend_composed)], iters, reps)
    row["blend_only"] = {"fused": cell(st["fused"]), "composed": cell(st["composed"]), "faster": verdict(st["fused"], st["composed"])}
    row["one_pass_mb"] = round(B * out * out * Cout * 4 / 1e6, 1)
    N._PAIR_FUSED = True
    return row


def generator_rows(B, mode, iters, reps):
    from vae_play_amd import network_Style_GAN as N
    torch.manual_seed(0)
    with torch.device("cuda"):
        g = N.Generator(256, 512)
    gen = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(B, 3, 256, 256, device="cuda", generator=gen).requires_grad_(True)
    style = torch.randn(B, 512, device="cuda", generator=gen).requires_grad_(True)
    gy = nhwc(B, 3, 256, gen)
    labels = torch.arange(B, device="cuda") % 2

    def whole(fused):
        def fn():
            N._PAIR_FUSED = fused
            g.zero_grad(set_to_none=True)
            x.grad = style.grad = None
            g(x, style, labels).backward(gy)
        return fn

    st = measure([("fused", whole(True)), ("composed", whole(False))], iters, reps)
    N._PAIR_FUSED = True
    return {"fused": cell(st["fused"]), "composed": cell(st["composed"]), "faster": verdict(st["fused"], st["composed"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r07_pairconv_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-generator", action="store_true", help="skip (b)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_pairconv needs a GPU: it measures nothing on the CPU")
    from vae_play_amd import functional as FH
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "image": 256, "iters_per_window": a.iters, "repetitions": a.reps,
           "method": "device events around windows of forward + backward passes through the autograd front end after warm-up; fused and "
                     "composed alternate; us = median [min, max] per forward + backward; 'faster' names a variant only where the "
                     "ranges do not overlap",
           "layers": {}, "generator_256_z512": {}}
    for mode in ("bf16x3", "f32"):
        FH.set_conv_precision(mode)
        for spec in LAYERS:
            row = layer_rows(*spec, a.batch, mode, a.iters, a.reps)
            res["layers"].setdefault(spec[0], {})[mode] = row
            print(spec[0], mode, json.dumps(row), flush=True)
            torch.cuda.empty_cache()
        if not a.no_generator:
            row = generator_rows(a.batch, mode, max(1, a.iters // 2), a.reps)
            res["generator_256_z512"][mode] = row
            print("generator", mode, json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    FH.set_conv_precision("f32")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
