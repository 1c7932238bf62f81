#!/usr/bin/env python
"""Inference benchmark: vae_play_amd.FusedVAEInference against the existing module path (``vae.eval()`` under ``torch.no_grad()``) in
ONE process, on the same weights and inputs.

For reconstruct, decode (= sample without the draw) and encode, at the benchmark shape (128x128x3, z = 128, batch 32) and at
config 2 (64x64x3, z = 64, batch 128), in both precisions: ms per call and images/s of
  modules      -- vae(x, eps) / vae.decoder(z) / vae.encoder(x), eval mode, no_grad, set_conv_precision(precision)
  fused        -- the pre-planned launch list, eager
  fused_graph  -- the same list replayed as a hipGraph
Each figure is the median over ``--reps`` windows of ``--iters`` calls, a window bracketed by device events on the launch stream
(so host-side gaps between launches are inside it: this is the time a caller waits, not kernel time); the variants alternate
inside every repetition, and min / max over the repetitions are reported as the spread.  Every variant is warmed up first.

``--layers`` adds, for every BatchNorm-followed 5x5 layer of the shape, the fused launch against convolution + normalise pass on
preallocated buffers (the per-layer evidence for which form the plan keeps).  ``--score K`` adds, at the benchmark shape, scored
images/s of ``FusedVAEInference.score`` with 1 and K draws per image (eager and replayed) against the composed path: the modules
in eval mode, then per-image BCE, density ratio and log-sum-exp in ATen (key ``score``; the other keys are unchanged).  The result
is one JSON document (``--out``).

With ``f16`` among ``--precisions`` (the one-product fp16 plans, which have no module path to stand against) the tool adds the
key ``modes``: per shape, ``reconstruct`` -- and with ``--score K`` also ``score`` with K draws -- of the plans of
every named precision over ONE model, eager and replayed, alternating in the same windows; per variant the median, min, max and the
spread max - min over the windows, and whether f16 beats bf16x3 by more than the sum of both spreads.  ``--layers`` then also lists
every 5x5 stride-2 layer's launch in f16 next to bf16x3 (key ``layers_f16``).  The module-path legs run for bf16x3 and f32 as before.

``--project STEPS`` adds, per shape and precision (bf16x3, f32), latent projection: ``FusedVAEInference.project`` with STEPS
iterations (eager, and replayed as a hipGraph) against the drop-in modules in ``.eval()`` under torch autograd with
``torch.optim.Adam`` on z (the decoder's parameters frozen, so autograd takes the input gradient alone), in the same alternating
windows: projections/s, microseconds per iteration, and whether the fused iteration is faster by more than the spread of the windows
(key ``project``).  Per launch of one iteration it also lists the time between device events around it (``launches``: where the
iteration's time goes).

``--vaegan`` adds the VAE-GAN leg (key ``vaegan``), at 128x128x1 batch 32 and 64x64x1 batch 128: ``FusedVAEGANInference.forward`` and
``.similarity``, eager and replayed, against the drop-in ``VaeGan`` in ``.eval()`` under ``set_conv_precision("bf16x3")`` computing the
same outputs (``net(x, eps=eps)``, ``discriminator.forward_rec_and_gan`` on (x, x_tilde), the loss terms with torch), in the same
alternating windows; and, with device events around each launch, the planes-writing stem against stem + split and the tap kernel
against the launches it replaces, at 2B rows.

    python tools/bench_infer.py --out bench_out/infer.json
    python tools/bench_infer.py --vaegan --vaegan-only --out bench_out/infer_vaegan.json
    python tools/bench_infer.py --project 20 --project-only --iters 5 --out bench_out/infer_project.json
    python tools/bench_infer.py --precisions f16,bf16x3,f32 --layers --score 8 --out bench_out/infer_f16.json
    python tools/bench_infer.py --score 8 --score-only --out bench_out/infer_score.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = {"bench_128x128x3_z128_b32": (3, 128, 128, 32), "config2_64x64x3_z64_b128": (3, 64, 64, 128)}


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def ab(variants, iters, reps, warmup):
    """variants: {name: fn}; alternated inside each repetition.  -> {name: {"ms": median, "min", "max"}}"""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(window(fn, iters))
    return {k: {"ms": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()}


def randomise_bn(vae, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in vae.modules():
            if hasattr(m, "num_batches_tracked"):
                m.weight.copy_(torch.empty(m.weight.shape).uniform_(0.5, 1.5, generator=g))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.empty(m.bias.shape).uniform_(0.5, 2.0, generator=g))


def bench_shape(name, C, S, z, B, prec, args):
    import vae_play_amd as V
    torch.manual_seed(0)
    vae = V.VAE(S, z, C).cuda().eval()
    randomise_bn(vae, 1)
    g = torch.Generator().manual_seed(2)
    x = torch.rand((B, C, S, S), generator=g).cuda()
    eps = torch.randn((B, z), generator=g).cuda()
    zz = torch.randn((B, z), generator=g).cuda()
    eager = V.FusedVAEInference(vae, B, S, C, precision=prec)
    graph = V.FusedVAEInference(vae, B, S, C, precision=prec)
    graph.capture()
    V.set_conv_precision(prec)
    out = {"fused_layers": eager.fused_layers, "unfused_layers": eager.unfused_layers}
    try:
        with torch.no_grad():
            # the three paths compute the same thing (recorded, not asserted: the parity tests assert)
            xm = vae(x, eps)[0]
            out["max_abs_diff_fused_vs_modules_x_tilde"] = (eager.reconstruct(x, eps)[0] - xm).abs().max().item()
            out["graph_equals_eager"] = bool(torch.equal(graph.reconstruct(x, eps)[0], eager.reconstruct(x, eps)[0]))
            ops_ = {
                "reconstruct": {"modules": lambda: vae(x, eps), "fused": lambda: eager.reconstruct(x, eps),
                                "fused_graph": lambda: graph.reconstruct(x, eps)},
                "decode": {"modules": lambda: vae.decoder(zz), "fused": lambda: eager.decode(zz), "fused_graph": lambda: graph.decode(zz)},
                "encode": {"modules": lambda: vae.encoder(x), "fused": lambda: eager.encode(x), "fused_graph": lambda: graph.encode(x)},
            }
            for op, variants in ops_.items():
                r = ab(variants, args.iters, args.reps, args.warmup)
                for v in r.values():
                    v["images_per_s"] = B / (v["ms"] * 1e-3)
                r["saved_ms_fused_vs_modules"] = r["modules"]["ms"] - r["fused"]["ms"]
                r["saved_ms_graph_vs_modules"] = r["modules"]["ms"] - r["fused_graph"]["ms"]
                out[op] = r
                print(f"{name} {prec} {op}: modules {r['modules']['ms']:.3f} ms [{r['modules']['min']:.3f}, {r['modules']['max']:.3f}]  "
                      f"fused {r['fused']['ms']:.3f} [{r['fused']['min']:.3f}, {r['fused']['max']:.3f}]  "
                      f"graph {r['fused_graph']['ms']:.3f} [{r['fused_graph']['min']:.3f}, {r['fused_graph']['max']:.3f}]", flush=True)
    finally:
        V.set_conv_precision("f32")
    return out


def bench_score(name, C, S, z, B, prec, args):
    """``--score K``: scored images/s with 1 and K draws per image -- FusedVAEInference.score (eager, and replayed as a hipGraph)
    against the composed path in the same process: the modules in eval mode (encoder once, reparameterise + decoder per draw),
    then per-image BCE, density ratio and log-sum-exp in ATen"""
    import math
    import torch.nn.functional as F
    import vae_play_amd as V
    torch.manual_seed(0)
    vae = V.VAE(S, z, C).cuda().eval()
    randomise_bn(vae, 1)
    g = torch.Generator().manual_seed(2)
    x = torch.rand((B, C, S, S), generator=g).cuda()
    out = {}
    V.set_conv_precision(prec)
    try:
        with torch.no_grad():
            for k in sorted({1, args.score}):
                eps = torch.randn((B, k, z), generator=g).cuda()
                eps_k = [eps[:, j].contiguous() for j in range(k)]
                eager = V.FusedVAEInference(vae, B, S, C, precision=prec)
                graph = V.FusedVAEInference(vae, B, S, C, precision=prec)
                graph.enable_scoring(k)
                graph.score(x, k, eps)
                graph.capture()

                def composed():
                    mu, logvar = vae.encoder(x)
                    kl = -0.5 * (1.0 + logvar - mu * mu - torch.exp(logvar)).sum(1)
                    bce, lr = [], []
                    for e in eps_k:
                        zz = V.reparameterize(mu, logvar, eps=e)
                        bce.append(F.binary_cross_entropy(vae.decoder(zz), x, reduction="none").flatten(1).sum(1))
                        lr.append(-0.5 * (zz * zz).sum(1) + 0.5 * (e * e + logvar).sum(1))
                    bce, lr = torch.stack(bce, 1), torch.stack(lr, 1)
                    logw = lr - bce
                    return {"bce": bce, "kl": kl, "logw": logw, "elbo": -(bce.mean(1) + kl), "iwae": torch.logsumexp(logw, 1) - math.log(k)}

                ref, got = composed(), eager.score(x, k, eps)
                r = ab({"composed": composed, "fused": lambda: eager.score(x, k, eps), "fused_graph": lambda: graph.score(x, k, eps)},
                       args.iters, args.reps, args.warmup)
                for v in r.values():
                    v["scored_images_per_s"] = B / (v["ms"] * 1e-3)
                # the paths compute the same thing (recorded, not asserted: the parity tests assert)
                r["max_rel_diff_fused_vs_composed_iwae"] = ((got["iwae"] - ref["iwae"]).abs() / ref["iwae"].abs()).max().item()
                # graph against eager AFTER the timing loops: a replay was seen to drift from the eager list with such a history
                #  while it is bit-identical right after capture()
                after_e, after_g = eager.score(x, k, eps), graph.score(x, k, eps)
                r["graph_equals_eager"] = all(bool(torch.equal(after_g[t], after_e[t])) for t in after_e)
                r["eager_equals_its_first_call"] = all(bool(torch.equal(after_e[t], got[t])) for t in got)
                r["max_rel_diff_graph_vs_eager"] = {t: ((after_g[t] - after_e[t]).abs() / after_e[t].abs()).max().item() for t in after_e}
                out[f"k{k}"] = r
                print(f"{name} {prec} score k={k}: composed {r['composed']['ms']:.3f} ms [{r['composed']['min']:.3f}, {r['composed']['max']:.3f}]  "
                      f"fused {r['fused']['ms']:.3f} [{r['fused']['min']:.3f}, {r['fused']['max']:.3f}]  "
                      f"graph {r['fused_graph']['ms']:.3f} [{r['fused_graph']['min']:.3f}, {r['fused_graph']['max']:.3f}]", flush=True)
    finally:
        V.set_conv_precision("f32")
    return out


def project_launches(inf, reps=5):
    """per launch of the "project" list: median microseconds between device events around it, in launch order"""
    names = {c[0] for p in inf._plans["project"] for c in p.calls}
    runs = []
    for _ in range(reps):
        timers = {"names": names, "events": []}
        s = torch.cuda.current_stream().cuda_stream
        for p in inf._plans["project"]:
            p.run(s, timers=timers)
        torch.cuda.synchronize()
        runs.append([(n, tag, e0.elapsed_time(e1) * 1e3) for n, tag, _, e0, e1 in timers["events"]])
    return [{"launch": n, "tag": tag, "us": statistics.median(r[i][2] for r in runs)} for i, (n, tag, _) in enumerate(runs[0])]


def bench_project(name, C, S, z, B, prec, args):
    """``--project STEPS``: FusedVAEInference.project (eager, replayed) against the modules in eval mode under torch autograd with
    torch.optim.Adam on z, all from the same z0 towards the same target, in alternating windows"""
    import torch.nn.functional as F
    import vae_play_amd as V
    steps, lr, pw = args.project, 0.05, 1.0
    torch.manual_seed(0)
    vae = V.VAE(S, z, C).cuda().eval()
    randomise_bn(vae, 1)
    g = torch.Generator().manual_seed(2)
    z0 = torch.randn((B, z), generator=g).cuda()
    eager = V.FusedVAEInference(vae, B, S, C, precision=prec)
    x = eager.decode(torch.randn((B, z), generator=g).cuda())         # a target the model can reach
    graph = V.FusedVAEInference(vae, B, S, C, precision=prec)
    graph.enable_projection()
    graph.capture()
    frozen = [p for p in vae.decoder.parameters() if p.requires_grad]
    for p in frozen:
        p.requires_grad_(False)
    V.set_conv_precision(prec)

    def modules():
        zt = z0.clone().requires_grad_(True)
        opt = torch.optim.Adam([zt], lr=lr)
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            loss = F.binary_cross_entropy(vae.decoder(zt), x, reduction="sum") + 0.5 * pw * (zt * zt).sum()
            loss.backward()
            opt.step()
        with torch.no_grad():
            xt = vae.decoder(zt)
            return zt.detach(), xt, F.binary_cross_entropy(xt, x, reduction="none").flatten(1).sum(1) + 0.5 * pw * (zt * zt).sum(1)

    try:
        kw = dict(steps=steps, lr=lr, z0=z0, prior_weight=pw)
        ref, got = modules(), eager.project(x, **kw)
        r = _with_spread(ab({"modules_autograd": modules, "fused": lambda: eager.project(x, **kw),
                             "fused_graph": lambda: graph.project(x, **kw)}, args.iters, args.reps, args.warmup), B, "projections_per_s")
        for v in r.values():
            v["us_per_iteration"] = v["ms"] * 1e3 / steps
        out = dict(r)
        out["steps"] = steps
        # the paths compute the same thing (recorded, not asserted: the parity tests assert)
        out["max_rel_diff_fused_vs_modules_loss"] = ((got["loss"] - ref[2]).abs() / ref[2].abs()).max().item()
        out["max_abs_diff_fused_vs_modules_z"] = (got["z"] - ref[0]).abs().max().item()
        # graph against eager AFTER the timing loops, as the scoring leg does, and a graph captured only now
        after_e, after_g = eager.project(x, **kw), graph.project(x, **kw)
        fresh = V.FusedVAEInference(vae, B, S, C, precision=prec)
        fresh.enable_projection()
        fresh.capture()
        after_f = fresh.project(x, **kw)
        out["graph_equals_eager"] = all(bool(torch.equal(after_g[k], after_e[k])) for k in after_e)
        out["fresh_graph_equals_eager"] = all(bool(torch.equal(after_f[k], after_e[k])) for k in after_e)
        out["eager_equals_its_first_call"] = all(bool(torch.equal(after_e[k], got[k])) for k in got)
        out["max_abs_diff_graph_vs_eager"] = {k: (after_g[k] - after_e[k]).abs().max().item() for k in after_e}
        for k in ("fused", "fused_graph"):
            saved, spread = r["modules_autograd"]["ms"] - r[k]["ms"], r["modules_autograd"]["spread_ms"] + r[k]["spread_ms"]
            out[k + "_vs_modules"] = {"speedup": r["modules_autograd"]["ms"] / r[k]["ms"], "saved_ms": saved, "sum_of_spreads_ms": spread,
                                      "faster_by_more_than_spreads": bool(saved > spread)}
        out["launches"] = project_launches(eager)
        for k in ("modules_autograd", "fused", "fused_graph"):
            v = r[k]
            print(f"{name} {prec} project x{steps} {k}: {v['ms']:.2f} ms [{v['min']:.2f}, {v['max']:.2f}]  {v['us_per_iteration']:.0f} us/iteration  "
                  f"{v['projections_per_s']:.0f} projections/s", flush=True)
        top = max(out["launches"], key=lambda c: c["us"])
        print(f"{name} {prec} project: fused vs modules {out['fused_vs_modules']}; largest launch {top}", flush=True)
    finally:
        V.set_conv_precision("f32")
        for p in frozen:
            p.requires_grad_(True)
    return out


def bench_layers(C, S, z, B, prec, args):
    """fused launch vs convolution + normalise pass, per BatchNorm-followed 5x5 layer, on preallocated buffers"""
    import vae_play_amd as V
    from vae_play_amd import _lib, ops
    from ctypes import c_void_p
    lib = _lib.load()
    vae = V.VAE(S, z, C)
    L = vae.iter_level
    enc_ch = [C] + [blk.conv.weight.shape[0] for blk in vae.encoder.conv]
    dec_ch = [vae.decoder._c0] + [blk.conv.weight.shape[1] for blk in list(vae.decoder.conv)[:L]]
    layers = [(f"enc{i}", 0, S >> (i + 1), enc_ch[i], enc_ch[i + 1]) for i in range(1, L)]
    layers += [(f"dec{i}", 1, 8 << i, dec_ch[i], dec_ch[i + 1]) for i in range(L)]
    res = {}
    P = lambda t: None if t is None else c_void_p(t.data_ptr())      # noqa: E731
    for tag, fam, Hs, Cin, Cout in layers:
        Cbig, Csmall = (Cin, Cout) if fam == 0 else (Cout, Cin)
        if not ops.conv5_affine_supported(fam, prec, B, Hs, Hs, Cbig, Csmall, 2):
            res[tag] = {"fused": None, "note": "launch shape not fusable (its plain launch splits K)"}
            continue
        Hin = 2 * Hs if fam == 0 else Hs
        Ho = Hs if fam == 0 else 2 * Hs
        a = torch.randn((B, Cin, Hin, Hin), device="cuda").contiguous(memory_format=torch.channels_last)
        w = torch.randn((Cout, Cin, 5, 5) if fam == 0 else (Cin, Cout, 5, 5), device="cuda") / (25 * Cin) ** 0.5
        n_out = B * Ho * Ho * Cout
        last = tag == f"dec{L - 1}" or tag == f"enc{L - 1}" or prec == "f32"      # consumers that read fp32
        y = torch.empty(n_out, device="cuda")
        c = torch.empty(n_out, device="cuda")
        ys = None if last else ops.empty_split(n_out, a)
        ones, zeros = torch.ones(Cout, device="cuda"), torch.zeros(Cout, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        geom = (B, Hs, Hs, Cin, Cout, 2)
        if prec == "bf16x3":
            a_in, wp = ops.split_f32(a), ops.pack_w5_split(w, fam == 0, fam == 1)[fam]
        else:
            a_in, wp = a, ops.pack_w5(w, fam == 0, fam == 1)[fam]
        fn_f = getattr(lib, ("vp_conv5_gather_affine_", "vp_conv5_scatter_affine_")[fam] + prec)
        fn_c = getattr(lib, ("vp_conv5_gather_", "vp_conv5_scatter_")[fam] + prec)

        def fused():
            _lib.check(fn_f(P(a_in), P(wp), P(ones), P(zeros), None if ys is not None else P(y), P(ys), *geom, ops.ACT_RELU, c_void_p(s)))

        def separate():
            if fam == 0:
                _lib.check(fn_c(P(a_in), P(wp), None, P(c), *geom, ops.ACT_NONE, c_void_p(s)))
            else:
                _lib.check(fn_c(P(a_in), P(wp), P(c), *geom, c_void_p(s)))
            if ys is None:
                _lib.check(lib.vp_bn_act_fwd_f32(P(c), P(zeros), P(ones), P(ones), P(zeros), P(y), n_out // Cout, Cout, ops.ACT_RELU, 0.0, c_void_p(s)))
            else:
                _lib.check(lib.vp_bn_act_fwd_split_f32(P(c), P(zeros), P(ones), P(ones), P(zeros), None, P(ys), n_out // Cout, Cout,
                                                       ops.ACT_RELU, 0.0, c_void_p(s)))

        r = ab({"fused": fused, "conv_plus_pass": separate}, args.iters, args.reps, args.warmup)
        res[tag] = {"fused_us": r["fused"]["ms"] * 1e3, "fused_us_min_max": [r["fused"]["min"] * 1e3, r["fused"]["max"] * 1e3],
                    "conv_plus_pass_us": r["conv_plus_pass"]["ms"] * 1e3,
                    "conv_plus_pass_us_min_max": [r["conv_plus_pass"]["min"] * 1e3, r["conv_plus_pass"]["max"] * 1e3],
                    "writes": "fp32" if ys is None else "split planes"}
        print(f"  layer {tag} {prec}: fused {res[tag]['fused_us']:.1f} us  conv + pass {res[tag]['conv_plus_pass_us']:.1f} us", flush=True)
    return res


def _with_spread(r, B, key):
    for v in r.values():
        v["spread_ms"] = v["max"] - v["min"]
        v[key] = B / (v["ms"] * 1e-3)
    return r


def _f16_verdict(r, suffix):
    """is f16 faster than bf16x3 by more than the sum of both variants' window-to-window spreads?"""
    f, b = r.get("f16" + suffix), r.get("bf16x3" + suffix)
    if f is None or b is None:
        return None
    return {"saved_ms": b["ms"] - f["ms"], "sum_of_spreads_ms": f["spread_ms"] + b["spread_ms"], "speedup": b["ms"] / f["ms"],
            "faster_by_more_than_spreads": bool(b["ms"] - f["ms"] > f["spread_ms"] + b["spread_ms"])}


def bench_modes(name, C, S, z, B, precs, args, score_k=0):
    """the plans of ``precs`` over one model in alternating windows: reconstruct, and score with ``score_k`` draws"""
    import vae_play_amd as V
    torch.manual_seed(0)
    vae = V.VAE(S, z, C).cuda().eval()
    randomise_bn(vae, 1)
    g = torch.Generator().manual_seed(2)
    x = torch.rand((B, C, S, S), generator=g).cuda()
    eps = torch.randn((B, z), generator=g).cuda()
    eager = {p: V.FusedVAEInference(vae, B, S, C, precision=p) for p in precs}
    graph = {p: V.FusedVAEInference(vae, B, S, C, precision=p) for p in precs}
    out = {}
    if score_k:
        eps_k = torch.randn((B, score_k, z), generator=g).cuda()
        for p in precs:
            graph[p].score(x, score_k, eps_k)
    for p in precs:
        graph[p].capture()
    base = eager[precs[-1]].reconstruct(x, eps)[0]      # (recorded, not asserted: the parity tests assert)
    out["max_abs_diff_x_tilde_vs_" + precs[-1]] = {p: (eager[p].reconstruct(x, eps)[0] - base).abs().max().item() for p in precs}
    variants = {}
    for p in precs:
        variants[p] = (lambda q: lambda: eager[q].reconstruct(x, eps))(p)
        variants[p + "_graph"] = (lambda q: lambda: graph[q].reconstruct(x, eps))(p)
    r = _with_spread(ab(variants, args.iters, args.reps, args.warmup), B, "images_per_s")
    out["reconstruct"] = r
    out["reconstruct_f16_vs_bf16x3"] = {"eager": _f16_verdict(r, ""), "graph": _f16_verdict(r, "_graph")}
    for k, v in r.items():
        print(f"{name} modes reconstruct {k}: {v['ms']:.3f} ms [{v['min']:.3f}, {v['max']:.3f}]  {v['images_per_s']:.0f} images/s", flush=True)
    print(f"{name} modes reconstruct f16 vs bf16x3: {out['reconstruct_f16_vs_bf16x3']}", flush=True)
    if score_k:
        variants = {}
        for p in precs:
            variants[p] = (lambda q: lambda: eager[q].score(x, score_k, eps_k))(p)
            variants[p + "_graph"] = (lambda q: lambda: graph[q].score(x, score_k, eps_k))(p)
        r = _with_spread(ab(variants, args.iters, args.reps, args.warmup), B, "scored_images_per_s")
        out[f"score_k{score_k}"] = r
        out[f"score_k{score_k}_f16_vs_bf16x3"] = {"eager": _f16_verdict(r, ""), "graph": _f16_verdict(r, "_graph")}
        for k, v in r.items():
            print(f"{name} modes score k={score_k} {k}: {v['ms']:.3f} ms [{v['min']:.3f}, {v['max']:.3f}]  {v['scored_images_per_s']:.0f} images/s",
                  flush=True)
    return out


def bench_layers_f16(C, S, z, B, args):
    """every 5x5 stride-2 layer of the shape as the f16 plan launches it next to the bf16x3 plan's launch: the fused launch where the
    shape fuses (f16 writes the hi plane, bf16x3 both planes; fp32 for the layers whose consumer reads fp32), else the plain
    convolution (the normalise pass that follows is the same kernel in both plans)"""
    import vae_play_amd as V
    from vae_play_amd import _lib, ops
    from ctypes import c_void_p
    lib = _lib.load()
    vae = V.VAE(S, z, C)
    L = vae.iter_level
    enc_ch = [C] + [blk.conv.weight.shape[0] for blk in vae.encoder.conv]
    dec_ch = [vae.decoder._c0] + [blk.conv.weight.shape[1] for blk in list(vae.decoder.conv)[:L]]
    layers = [(f"enc{i}", 0, S >> (i + 1), enc_ch[i], enc_ch[i + 1]) for i in range(1, L)]
    layers += [(f"dec{i}", 1, 8 << i, dec_ch[i], dec_ch[i + 1]) for i in range(L)]
    res = {}
    P = lambda t: None if t is None else c_void_p(t.data_ptr())      # noqa: E731
    for tag, fam, Hs, Cin, Cout in layers:
        Cbig, Csmall = (Cin, Cout) if fam == 0 else (Cout, Cin)
        fusable = ops.conv5_affine_supported(fam, "f16", B, Hs, Hs, Cbig, Csmall, 2)
        Hin, Ho = (2 * Hs, Hs) if fam == 0 else (Hs, 2 * Hs)
        a = torch.randn((B, Cin, Hin, Hin), device="cuda").contiguous(memory_format=torch.channels_last)
        w = torch.randn((Cout, Cin, 5, 5) if fam == 0 else (Cin, Cout, 5, 5), device="cuda") / (25 * Cin) ** 0.5
        n_out = B * Ho * Ho * Cout
        last = tag in (f"dec{L - 1}", f"enc{L - 1}")      # consumers that read fp32
        y = torch.empty(n_out, device="cuda")
        ys = None if last else ops.empty_split(n_out, a)
        ones, zeros = torch.ones(Cout, device="cuda"), torch.zeros(Cout, device="cuda")
        s = c_void_p(torch.cuda.current_stream().cuda_stream)
        geom = (B, Hs, Hs, Cin, Cout, 2)
        ab16, wb16 = ops.split_f32(a), ops.pack_w5_split(w, fam == 0, fam == 1)[fam]
        ah16, wh16 = ops.split_f32(a, ops.SPLIT_F16), ops.pack_w5_split(w, fam == 0, fam == 1, ops.SPLIT_F16)[fam]
        fam_name = ("gather", "scatter")[fam]
        yo = None if ys is not None else P(y)
        if fusable:
            fn_h, fn_b = getattr(lib, f"vp_conv5_{fam_name}_affine_f16"), getattr(lib, f"vp_conv5_{fam_name}_affine_bf16x3")
            fmt = ops.OUT_BF16_PAIR if tag == f"dec{L - 1}" else ops.OUT_F16_HI
            variants = {"f16": lambda: _lib.check(fn_h(P(ah16), P(wh16), P(ones), P(zeros), yo, P(ys), *geom, ops.ACT_RELU, fmt, s)),
                        "bf16x3": lambda: _lib.check(fn_b(P(ab16), P(wb16), P(ones), P(zeros), yo, P(ys), *geom, ops.ACT_RELU, s))}
        else:
            fn_h, fn_b = getattr(lib, f"vp_conv5_{fam_name}_f16"), getattr(lib, f"vp_conv5_{fam_name}_bf16x3")
            if fam == 0:
                variants = {"f16": lambda: _lib.check(fn_h(P(ah16), P(wh16), None, P(y), *geom, ops.ACT_NONE, 1, 1.0, s)),
                            "bf16x3": lambda: _lib.check(fn_b(P(ab16), P(wb16), None, P(y), *geom, ops.ACT_NONE, s))}
            else:
                variants = {"f16": lambda: _lib.check(fn_h(P(ah16), P(wh16), P(y), *geom, 1, 1.0, s)),
                            "bf16x3": lambda: _lib.check(fn_b(P(ab16), P(wb16), P(y), *geom, s))}
        r = ab(variants, args.iters, args.reps, args.warmup)
        res[tag] = {"launch": "fused" if fusable else "plain convolution (K is split: not fusable)",
                    "f16_us": r["f16"]["ms"] * 1e3, "f16_us_min_max": [r["f16"]["min"] * 1e3, r["f16"]["max"] * 1e3],
                    "bf16x3_us": r["bf16x3"]["ms"] * 1e3, "bf16x3_us_min_max": [r["bf16x3"]["min"] * 1e3, r["bf16x3"]["max"] * 1e3],
                    "speedup": r["bf16x3"]["ms"] / r["f16"]["ms"], "gflop": 50.0 * B * Hs * Hs * Cin * Cout * 1e-9,
                    "writes": "fp32" if ys is None else "f16: hi plane; bf16x3: both planes"}
        print(f"  layer {tag}: f16 {res[tag]['f16_us']:.1f} us  bf16x3 {res[tag]['bf16x3_us']:.1f} us  ({res[tag]['speedup']:.2f}x, {res[tag]['launch']})",
              flush=True)
    return res


VAEGAN_SHAPES = {"vaegan_128x128x1_z128_b32": (128, 128, 32), "vaegan_64x64x1_z64_b128": (64, 64, 128)}      # (S, z, B)


def _launch_ab(variants, args):
    """{name: [launch, ...]} with device events around EACH launch, the variants alternating: per variant the summed medians of its
    launches in microseconds, min and max of the per-repetition sums"""
    def once(fns):
        ev = []
        for fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
    for fns in variants.values():
        for _ in range(args.warmup):
            once(fns)
    t = {k: [] for k in variants}
    for _ in range(args.reps * args.iters):
        for k, fns in variants.items():
            t[k].append(once(fns))
    out = {}
    for k, runs in t.items():
        sums = [sum(r) for r in runs]
        out[k] = {"us": statistics.median(sums), "min": min(sums), "max": max(sums),
                  "per_launch_us": [statistics.median(r[i] for r in runs) for i in range(len(runs[0]))]}
    return out


def bench_vaegan_kernels(S, B, Cd):
    """the launches for the A/B of the two fused kernels at 2B rows: the planes-writing stem against stem + split, the tap kernel
    against normalise pass + two transposes + row sum"""
    from vae_play_amd import _lib, ops
    from ctypes import c_void_p
    lib = _lib.load()
    P = lambda t: None if t is None else c_void_p(t.data_ptr())      # noqa: E731
    s = c_void_p(torch.cuda.current_stream().cuda_stream)
    n2, C0 = 2 * B, 32
    x = torch.rand((n2, 1, S, S), device="cuda")
    w, bias = torch.randn((C0, 1, 5, 5), device="cuda") * 0.1, torch.randn(C0, device="cuda") * 0.1
    n0 = n2 * S * S * C0
    y0, y0s = torch.empty(n0, device="cuda"), torch.empty((2, n0), dtype=torch.int16, device="cuda")
    half = n0 // 2
    stem = {
        "planes_two_halves": [lambda k=k: _lib.check(lib.vp_conv5_smallin_fwd_planes_bf16x3(
            c_void_p(x.data_ptr() + 4 * k * B * S * S), P(w), P(bias), c_void_p(y0s.data_ptr() + 2 * k * half), n0, B, S, S, 1, C0,
            ops.ACT_RELU, s)) for k in range(2)],
        "fp32_then_split": [lambda: _lib.check(lib.vp_conv5_smallin_fwd_bf16x3(P(x), P(w), P(bias), P(y0), n2, S, S, 1, C0, ops.ACT_RELU, s)),
                            lambda: _lib.check(lib.vp_split_f32(P(y0), P(y0s), n0, s))],
    }
    c = torch.randn((n2, 64, Cd), device="cuda")
    a, act, feat = torch.empty_like(c), torch.empty((n2, Cd * 64), device="cuda"), torch.empty((n2, Cd * 64), device="cuda")
    sc, sh = torch.rand(Cd, device="cuda") + 0.5, torch.randn(Cd, device="cuda")
    zeros, ones, dist = torch.zeros(Cd, device="cuda"), torch.ones(Cd, device="cuda"), torch.empty(B, device="cuda")
    tap = {
        "tap_kernel": [lambda: _lib.check(lib.vp_disc_tap_eval_f32(P(c), P(sc), P(sh), n2, Cd, P(act), None, B, P(dist), s))],
        "pass_transpose_rowsum": [
            lambda: _lib.check(lib.vp_bn_act_fwd_f32(P(c), P(zeros), P(ones), P(sc), P(sh), P(a), n2 * 64, Cd, ops.ACT_RELU, 0.0, s)),
            lambda: _lib.check(lib.vp_nhwc_to_nchw_f32(P(a), P(act), n2, Cd, 8, 8, s)),
            lambda: _lib.check(lib.vp_half_sqdiff_rowsum_f32(P(c), c_void_p(c.data_ptr() + 4 * B * 64 * Cd), P(dist), B, 64 * Cd, s))],
    }
    return stem, tap


def bench_vaegan(name, S, z, B, args):
    """``--vaegan``: FusedVAEGANInference.forward and .similarity (eager, and replayed as a hipGraph) against the drop-in VaeGan in
    ``.eval()`` under set_conv_precision("bf16x3") computing the same outputs -- net(x, eps=eps), forward_rec_and_gan on
    (x, x_tilde), the loss terms with torch -- in alternating windows; then the two fused kernels against the launches they replace"""
    import vae_play_amd as V
    torch.manual_seed(0)
    net = V.VaeGan(S, z).cuda().eval()
    randomise_bn(net, 1)
    g = torch.Generator().manual_seed(2)
    x = torch.rand((B, 1, S, S), generator=g).cuda()
    eps = torch.randn((B, z), generator=g).cuda()
    eager, graph = V.FusedVAEGANInference(net, B), V.FusedVAEGANInference(net, B)
    graph.enable_gan()
    graph.capture()
    none = x[:0]

    def modules_forward():
        return net(x, eps=eps)

    def modules_similarity():
        xt, params = net(x, eps=eps)
        feat, p = net.discriminator.forward_rec_and_gan(x, xt, none)
        p = p.reshape(-1)
        return {"x_tilde": xt, "params": params, "nle": (0.5 * (x - xt) ** 2).flatten(1).sum(1),
                "mse": (0.5 * (feat[:B] - feat[B:]) ** 2).sum(1), "p_x": p[:B], "p_x_tilde": p[B:],
                "bce_dis_original": -torch.log(p[:B] + 1e-3), "bce_dis_predicted": -torch.log(1 - p[B:] + 1e-3)}
    out = {}
    V.set_conv_precision("bf16x3")
    try:
        with torch.no_grad():
            ref, got = modules_similarity(), eager.similarity(x, eps)
            # the paths compute the same thing (recorded, not asserted: the parity tests assert)
            out["max_rel_diff_fused_vs_modules"] = {k: ((got[k] - ref[k]).abs().max() / ref[k].abs().max()).item() for k in ref}
            legs = {"forward": {"modules": modules_forward, "fused": lambda: eager.forward(x, eps), "fused_graph": lambda: graph.forward(x, eps)},
                    "similarity": {"modules": modules_similarity, "fused": lambda: eager.similarity(x, eps),
                                   "fused_graph": lambda: graph.similarity(x, eps)}}
            for leg, variants in legs.items():
                r = _with_spread(ab(variants, args.iters, args.reps, args.warmup), B, "images_per_s")
                res = dict(r)
                for k in ("fused", "fused_graph"):
                    saved, spread = r["modules"]["ms"] - r[k]["ms"], r["modules"]["spread_ms"] + r[k]["spread_ms"]
                    res[k + "_vs_modules"] = {"speedup": r["modules"]["ms"] / r[k]["ms"], "saved_ms": saved, "sum_of_spreads_ms": spread,
                                              "faster_by_more_than_spreads": bool(saved > spread)}
                out[leg] = res
                print(f"{name} {leg}: modules {r['modules']['ms']:.3f} ms [{r['modules']['min']:.3f}, {r['modules']['max']:.3f}]  "
                      f"fused {r['fused']['ms']:.3f} [{r['fused']['min']:.3f}, {r['fused']['max']:.3f}]  "
                      f"graph {r['fused_graph']['ms']:.3f} [{r['fused_graph']['min']:.3f}, {r['fused_graph']['max']:.3f}]  "
                      f"fused x{res['fused_vs_modules']['speedup']:.2f} graph x{res['fused_graph_vs_modules']['speedup']:.2f}", flush=True)
            # graph against eager AFTER the timing loops, as the scoring leg does
            after_e, after_g = eager.similarity(x, eps), graph.similarity(x, eps)
            out["graph_equals_eager"] = all(bool(torch.equal(after_g[k], after_e[k])) for k in after_e)
            out["eager_equals_its_first_call"] = all(bool(torch.equal(after_e[k], got[k])) for k in got)
            stem, tap = bench_vaegan_kernels(S, B, eager._gan.disc.Cd)
            for what, variants in (("stem", stem), ("tap", tap)):
                r = _launch_ab(variants, args)
                (new, rn), (old, ro) = r.items()
                r["saved_us"], r["sum_of_spreads_us"] = ro["us"] - rn["us"], (rn["max"] - rn["min"]) + (ro["max"] - ro["min"])
                r["faster_by_more_than_spreads"] = bool(r["saved_us"] > r["sum_of_spreads_us"])
                out["kernel_" + what] = r
                print(f"{name} kernel {what}: {new} {rn['us']:.1f} us [{rn['min']:.1f}, {rn['max']:.1f}]  {old} {ro['us']:.1f} us "
                      f"[{ro['min']:.1f}, {ro['max']:.1f}]  per launch {rn['per_launch_us']} vs {ro['per_launch_us']}", flush=True)
    finally:
        V.set_conv_precision("f32")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=40, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=5, help="windows per variant (alternating)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", action="store_true", help="per-layer fused launch vs convolution + normalise pass")
    ap.add_argument("--score", type=int, default=0, metavar="K",
                    help="add the scoring leg at 128x128x3 batch 32: score() with 1 and K draws against the composed path")
    ap.add_argument("--score-only", action="store_true", help="with --score: skip the reconstruct / decode / encode legs")
    ap.add_argument("--project", type=int, default=0, metavar="STEPS",
                    help="add the projection leg: project() with STEPS iterations against the modules under autograd + torch.optim.Adam")
    ap.add_argument("--project-only", action="store_true", help="with --project: skip every other leg")
    ap.add_argument("--vaegan", action="store_true",
                    help="add the VAE-GAN leg (128x128x1 batch 32, 64x64x1 batch 128): FusedVAEGANInference forward / similarity "
                         "against the drop-in VaeGan in eval mode, and the two fused kernels against the launches they replace")
    ap.add_argument("--vaegan-only", action="store_true", help="with --vaegan: skip every other leg")
    ap.add_argument("--shapes", default=",".join(SHAPES), help="comma-separated subset of: " + ", ".join(SHAPES))
    ap.add_argument("--precisions", default="bf16x3,f32", help="comma-separated subset of: f16, bf16x3, f32")
    ap.add_argument("--out", default="bench_out/infer.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_infer.py measures on the GPU; none is visible")
    doc = {"tool": "tools/bench_infer.py", "device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps,
           "timing": "device events around a window of calls (host gaps included); median [min, max] over alternating repetitions",
           "results": {}, "layers": {}}
    if args.score < 0 or (args.score_only and not args.score):
        raise SystemExit("--score takes a positive K; --score-only needs it")
    precs = args.precisions.split(",")
    if any(p not in ("f16", "bf16x3", "f32") for p in precs):
        raise SystemExit("--precisions takes f16, bf16x3, f32")
    module_precs = [p for p in precs if p != "f16"]      # (the module path has no one-product mode to compare against)
    if args.project < 0 or (args.project_only and not args.project):
        raise SystemExit("--project takes a positive STEPS; --project-only needs it")
    if args.vaegan_only and not args.vaegan:
        raise SystemExit("--vaegan-only needs --vaegan")
    if args.vaegan:
        doc["vaegan"] = {name: bench_vaegan(name, *shape, args) for name, shape in VAEGAN_SHAPES.items()}
    if args.vaegan_only:
        args.project = args.score = 0
        precs = module_precs = []
        args.score_only = True          # (no reconstruct / decode / encode legs)
    if args.project:
        doc["project"] = {}
        for name in args.shapes.split(","):
            for prec in module_precs:       # ("f16" plans refuse projection)
                doc["project"][f"{name}/{prec}"] = bench_project(name, *SHAPES[name], prec, args)
    if "f16" in precs and not args.project_only:      # first: the alternating-window comparison of the modes, before the long module-path legs
        doc["modes"], doc["layers_f16"] = {}, {}
        for name in args.shapes.split(","):
            C, S, z, B = SHAPES[name]
            doc["modes"][name] = bench_modes(name, C, S, z, B, precs, args, args.score)
            if args.layers:
                doc["layers_f16"][name] = bench_layers_f16(C, S, z, B, args)
    if args.score and not args.project_only:
        doc["score"] = {}
        name = "bench_128x128x3_z128_b32"
        for prec in module_precs:
            doc["score"][f"{name}/{prec}"] = bench_score(name, *SHAPES[name], prec, args)
    for name in args.shapes.split(",") if not (args.score_only or args.project_only) else ():
        C, S, z, B = SHAPES[name]
        for prec in module_precs:
            doc["results"][f"{name}/{prec}"] = bench_shape(name, C, S, z, B, prec, args)
            if args.layers:
                doc["layers"][f"{name}/{prec}"] = bench_layers(C, S, z, B, prec, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
