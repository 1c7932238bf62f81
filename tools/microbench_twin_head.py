"""The Style-GAN discriminator's output stage (models/network_Style_GAN.py:214-229), fused against composed: functional.twin_head (one
launch forward, one backward) against the reference's expression over two Conv2d blocks, a sigmoid and a row softmax, forward +
backward through the autograd front end, in bf16x3 and f32.
usage: python tools/microbench_twin_head.py [--out profiles/r08_twin_head_bench.json] [--batch 32] [--iters 5] [--reps 7] [--no-networks]

  (a) stage          the output stage alone on given (B, C, 2, 2) head activations at (B, C, K) = (batch, 256, 2)
  (b) discriminator  Discriminator(256, 2) forward + backward with network_Style_GAN._HEAD_FUSED on and off
  (c) encoder        StyleEncoder(512, 256) forward + backward, for the record (it has no switch)

Method: one process; device events around windows of --iters forward + backward passes after a warm-up of both variants; the variants
alternate, --reps repetitions each; median [min, max] in microseconds per forward + backward."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


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
    """DESIGN.md section 16(b)'s rule: a variant is named only where its [min, max] lies wholly below the other's"""
    if fused[2] < composed[1]:
        return "fused"
    if composed[2] < fused[1]:
        return "composed"
    return "inside the spread"


def pair(st):
    return {"fused": cell(st["fused"]), "composed": cell(st["composed"]), "faster": verdict(st["fused"], st["composed"])}


def nhwc(B, C, H, gen):
    return torch.randn(B, H, H, C, device="cuda", generator=gen).permute(0, 3, 1, 2)


def stage_row(B, C, K, iters, reps):
    from vae_play_amd import blocks, functional as FH
    gen = torch.Generator(device="cuda").manual_seed(1)
    torch.manual_seed(0)
    adv1, aux1 = blocks.Conv2d(C, 1, 3, stride=2, activate=None).cuda(), blocks.Conv2d(C, K, 3, stride=2, activate=None).cuda()
    pa, pu = adv1.conv[0], aux1.conv[0]
    h_adv, h_aux = nhwc(B, C, 2, gen).requires_grad_(True), nhwc(B, C, 2, gen).requires_grad_(True)
    g_adv, g_aux = torch.randn(B, 1, device="cuda", generator=gen), torch.randn(B, K, device="cuda", generator=gen)

    def run(fused):
        def fn():
            adv1.zero_grad(set_to_none=True)
            aux1.zero_grad(set_to_none=True)
            h_adv.grad = h_aux.grad = None
            if fused:
                adv, aux = FH.twin_head(h_adv, h_aux, pa.weight, pa.bias, pu.weight, pu.bias)
            else:
                adv = FH.activation(adv1(h_adv).reshape(B, -1), "sigmoid")
                aux = FH.softmax_rows(aux1(h_aux).reshape(B, -1))
            torch.autograd.backward([adv, aux], [g_adv, g_aux])
        return fn

    return pair(measure([("fused", run(True)), ("composed", run(False))], iters, reps))


def discriminator_row(B, iters, reps):
    from vae_play_amd import network_Style_GAN as N
    torch.manual_seed(0)
    with torch.device("cuda"):
        d = N.Discriminator(256, 2)
    gen = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(B, 3, 256, 256, device="cuda", generator=gen).requires_grad_(True)
    xc = torch.randn(B, 3, 256, 256, device="cuda", generator=gen)
    g_adv, g_aux = torch.randn(B, 1, device="cuda", generator=gen), torch.randn(B, 2, device="cuda", generator=gen)

    def run(fused):
        def fn():
            N._HEAD_FUSED = fused
            assert d.uses_fused_head(x, xc) == fused
            d.zero_grad(set_to_none=True)
            x.grad = None
            torch.autograd.backward(list(d(x, xc, None)), [g_adv, g_aux])
        return fn

    st = measure([("fused", run(True)), ("composed", run(False))], iters, reps)
    N._HEAD_FUSED = True
    return pair(st)


def encoder_row(B, iters, reps):
    from vae_play_amd import network_Style_GAN as N
    torch.manual_seed(0)
    with torch.device("cuda"):
        e = N.StyleEncoder(512, 256)
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, 3, 256, 256, device="cuda", generator=gen).requires_grad_(True)
    g_mu, g_lv = torch.randn(B, 512, device="cuda", generator=gen), torch.randn(B, 512, device="cuda", generator=gen)

    def fn():
        e.zero_grad(set_to_none=True)
        x.grad = None
        torch.autograd.backward(list(e(x)), [g_mu, g_lv])

    return cell(measure([("encoder", fn)], iters, reps)["encoder"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r08_twin_head_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-networks", action="store_true", help="skip (b) and (c)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_twin_head needs a GPU: it measures nothing on the CPU")
    from vae_play_amd import functional as FH
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "iters_per_window": a.iters, "repetitions": a.reps,
           "method": "device events around windows of forward + backward passes through the autograd front end after warm-up; fused and "
                     "composed alternate; us = median [min, max] per forward + backward; 'faster' names a variant only where the "
                     "ranges do not overlap",
           "stage_c256_k2": {}, "discriminator_256_k2": {}, "encoder_256_z512": {}}
    for mode in ("bf16x3", "f32"):
        FH.set_conv_precision(mode)
        res["stage_c256_k2"][mode] = stage_row(a.batch, 256, 2, 10 * a.iters, a.reps)
        print("stage", mode, json.dumps(res["stage_c256_k2"][mode]), flush=True)
        if not a.no_networks:
            res["discriminator_256_k2"][mode] = discriminator_row(a.batch, a.iters, a.reps)
            print("discriminator", mode, json.dumps(res["discriminator_256_k2"][mode]), flush=True)
            torch.cuda.empty_cache()
            res["encoder_256_z512"][mode] = encoder_row(a.batch, a.iters, a.reps)
            print("encoder", mode, json.dumps(res["encoder_256_z512"][mode]), flush=True)
            torch.cuda.empty_cache()
    FH.set_conv_precision("f32")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
