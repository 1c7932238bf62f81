"""Style-GAN inference (train_Style_GAN.py:148-153,279-280): ``network_Style_GAN.Generator(S, z)`` / ``StyleEncoder`` / ``Discriminator``
on a batch of images, as
  modules  the drop-in modules under ``torch.no_grad()`` with ``set_conv_precision(prec)`` (the autograd front end),
  eager    ``FusedStyleGanInference`` running its launch lists,
  graph    the same after ``capture()`` (one hipGraph replay per call),
in ONE process, the three rows alternated over ``--rounds`` windows each; a window is as many calls as fill ``--window`` seconds and
ends in a device synchronise.  Reported per row: the median window's time per call and the spread (min, max) over the windows.  All
rows get the same channels_last inputs; the fused rows include the copies of the inputs into the plan's buffers and of the results out
of them.  Methods: generate with a label tensor, generate with the int label 1 (modules: a tensor of ones), stylize (eps=None),
encode_style, discriminate.
usage: python tools/bench_stylegan_infer.py [--sizes 256,128] [--z 512] [--batch 32] [--precisions f32,bf16x3] [--out FILE]
       python tools/bench_stylegan_infer.py --pieces [--sizes 256,128] [--out FILE]
``--pieces`` times no rows: vp_scse2_fwd_f32 next to two vp_scse_fwd_f32 calls at the three StyleUp shapes, vp_sg_out_tanh_f32 next to
the convolution + vp_act_fwd_f32 + vp_nhwc_to_nchw_f32 launches it replaces, and the folded MLP's dense launch next to the three
layers', each as a device event pair around ``--reps`` back-to-back calls, the two alternated over ``--rounds`` rounds; median and
spread.  Prints one JSON line (and writes it to --out)."""
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


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def ab_us(new, old, reps, rounds):
    """the two alternated: {"new_us", "new_min_max_us", "old_us", "old_min_max_us", "old_over_new", "new_wholly_below"}"""
    for _ in range(3):
        new()
        old()
    torch.cuda.synchronize()
    tn, to = [], []
    for _ in range(rounds):
        tn.append(event_ms(new, reps) * 1e3)
        to.append(event_ms(old, reps) * 1e3)
    return {"new_us": round(statistics.median(tn), 2), "new_min_max_us": [round(min(tn), 2), round(max(tn), 2)],
            "old_us": round(statistics.median(to), 2), "old_min_max_us": [round(min(to), 2), round(max(to), 2)],
            "old_over_new": round(statistics.median(to) / statistics.median(tn), 3), "new_wholly_below": max(tn) < min(to)}


def pieces(S, Z, B, reps, rounds):
    import vae_play_amd.infer_stylegan as IS
    from vae_play_amd import _lib, network_Style_GAN as N
    lib = _lib.load()
    P = lambda t: c_void_p(t.data_ptr())             # noqa: E731
    s = c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(3)
    rows = []
    # (a) the SCSE pair at the three StyleUp shapes of Generator(S, .)
    for C, side in ((256, S // 8), (128, S // 4), (64, S // 2)):
        HW, hid = side * side, C // 4
        x = torch.randn((B, HW, C), generator=g).to("cuda")
        par = [[(torch.rand(n, generator=g) - 0.5).to("cuda") for n in (hid * C, hid, C * hid, C, C, 1)] for _ in range(2)]
        y1, y2, mid = (torch.empty_like(x) for _ in range(3))
        pool, hb, cg, sg = (torch.empty(n, device="cuda") for n in (B * C, B * hid, B * C, B * HW))
        n2, n1 = lib.vp_scse2_workspace_bytes(B, HW, C, hid), lib.vp_scse_workspace_bytes(B, HW, C, hid)
        ws2, ws1 = torch.empty(n2 // 4 + 1, device="cuda"), torch.empty(n1 // 4 + 1, device="cuda")
        ys = torch.empty((2, x.numel()), dtype=torch.int16, device="cuda")
        pa, pb = [P(t) for t in par[0]], [P(t) for t in par[1]]

        def new(planes=None):
            _lib.check(lib.vp_scse2_fwd_f32(P(x), *pa, *pb, P(y1), planes, B, HW, C, hid, 1, P(ws2), n2, s), "scse2")

        def new_planes():
            new(P(ys))

        def old():
            _lib.check(lib.vp_scse_fwd_f32(P(x), *pa, P(mid), P(pool), P(hb), P(cg), P(sg), B, HW, C, hid, 0, P(ws1), n1, s), "scse")
            _lib.check(lib.vp_scse_fwd_f32(P(mid), *pb, P(y2), P(pool), P(hb), P(cg), P(sg), B, HW, C, hid, 1, P(ws1), n1, s), "scse")

        def old_planes():
            old()
            _lib.check(lib.vp_split_f32(P(y2), P(ys), x.numel(), s), "split")
        new()
        old()
        torch.cuda.synchronize()
        diff = float((y1 - y2).abs().max() / y2.abs().max())
        mb = x.numel() * 4 / 1e6
        rows.append({"piece": "scse2 vs 2 x scse", "B": B, "HW": f"{side}x{side}", "C": C, "tensor_MB": round(mb, 1), "max_rel_diff": diff,
                     "plan_uses_kernel": bool(lib.vp_scse2_preferred(B, HW, C, hid)), **ab_us(new, old, reps, rounds)})
        rows.append({"piece": "scse2 with planes vs 2 x scse + split", "B": B, "HW": f"{side}x{side}", "C": C, "tensor_MB": round(mb, 1),
                     **ab_us(new_planes, old_planes, reps, rounds)})
        del x, y1, y2, mid, ys
    # (c) final.3 + tanh
    C = 32
    x = torch.randn((B, S, S, C), generator=g).to("cuda")
    w, bias = ((torch.rand((3, C, 3, 3), generator=g) - 0.5) * 0.2).to("cuda"), torch.tensor([0.1, -0.2, 0.3]).to("cuda")
    par, p0 = torch.empty(lib.vp_sg_out_params_floats(C), device="cuda"), torch.empty((3, 9, C), device="cuda")
    _lib.check(lib.vp_sg_out_pack_f32(P(w), P(bias), P(par), C, s), "pack")
    _lib.check(lib.vp_pack_w_f32(P(w), P(p0), None, 3, C, 3, s), "pack")
    o1, o2, c = torch.empty((B, 3, S, S), device="cuda"), torch.empty((B, 3, S, S), device="cuda"), torch.empty((B, S, S, 3), device="cuda")

    def new():
        _lib.check(lib.vp_sg_out_tanh_f32(P(x), P(par), P(o1), B, S, S, C, s), "sg_out")

    def old():
        _lib.check(lib.vp_conv_gather_f32(P(x), P(p0), P(bias), P(c), B, S, S, S, S, C, 3, 3, 1, 0, s), "conv")
        _lib.check(lib.vp_act_fwd_f32(P(c), P(c), c.numel(), 3, 0.0, s), "tanh")
        _lib.check(lib.vp_nhwc_to_nchw_f32(P(c), P(o2), B, 3, S, S, s), "nchw")
    new()
    old()
    torch.cuda.synchronize()
    rows.append({"piece": "sg_out_tanh vs conv + tanh + transpose", "B": B, "HW": f"{S}x{S}", "C": C,
                 "max_rel_diff": float((o1 - o2).abs().max() / o2.abs().max()),
                 "plan_uses_kernel": bool(lib.vp_sg_out_tanh_preferred(B, S, S, C)), **ab_us(new, old, reps, rounds)})
    del x, o1, o2, c
    # the folded MLP's one dense launch next to the three layers' (the plans' own launch lists)
    torch.manual_seed(0)
    G = N.Generator(S, Z).to("cuda")
    keep = IS._mlp_fold_preferred
    plans, z0 = {}, torch.randn((B, Z), generator=g)
    try:
        for folded in (True, False):
            IS._mlp_fold_preferred = lambda *_a, _f=folded: _f
            inf = IS.FusedStyleGanInference(G, batch_size=B, precision="f32")
            inf.z.copy_(z0)
            plans[folded] = (inf, inf._plans["generate.blend"][0])
    finally:
        IS._mlp_fold_preferred = keep
    stream = torch.cuda.current_stream().cuda_stream
    new, old = (lambda: plans[True][1].run(stream)), (lambda: plans[False][1].run(stream))
    new()
    old()
    torch.cuda.synchronize()
    a, b = plans[True][0].style, plans[False][0].style
    weights_mb = sum(blk.fc[0].weight.numel() for blk in G.mlp.model) * 4 / 1e6
    rows.append({"piece": "folded MLP (1 dense launch) vs 3 layers", "B": B, "S": S, "z": Z, "three_layer_weights_MB": round(weights_mb, 1),
                 "folded_map_MB": round(S * S * Z * 4 / 1e6, 1), "max_rel_diff": float((a - b).abs().max() / b.abs().max()),
                 "plan_uses_fold": bool(keep(S, Z)), **ab_us(new, old, max(3, reps // 5), rounds)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,128")
    ap.add_argument("--z", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precisions", default="f32,bf16x3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of work per timed window")
    ap.add_argument("--pieces", action="store_true")
    ap.add_argument("--reps", type=int, default=30, help="--pieces: back-to-back calls inside one event pair")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stylegan_infer.py measures on the GPU; none is visible")
    import vae_play_amd as V
    from vae_play_amd import network_Style_GAN as N
    B, Z = a.batch, a.z
    rows_out = []
    for S in (int(v) for v in a.sizes.split(",")):
        if a.pieces:
            rows_out.append({"net": f"Generator({S}, {Z})", "batch": B, "pieces": pieces(S, Z, B, a.reps, a.rounds)})
            continue
        torch.manual_seed(0)
        G, E, D = N.Generator(S, Z).to("cuda"), N.StyleEncoder(Z, S).to("cuda"), N.Discriminator(S, 2).to("cuda")
        g = torch.Generator().manual_seed(1)
        xc, xs, x = (torch.rand((B, 3, S, S), generator=g).to("cuda").contiguous(memory_format=torch.channels_last) for _ in range(3))
        z, lab = torch.randn((B, Z), generator=g).to("cuda"), torch.randint(0, 2, (B,), generator=g).to("cuda")
        ones = torch.ones((B,), device="cuda")
        for prec in a.precisions.split(","):
            eager = V.FusedStyleGanInference(G, E, D, batch_size=B, precision=prec)
            graph = V.FusedStyleGanInference(G, E, D, batch_size=B, precision=prec)
            graph.capture()

            def modules(f):
                def run():
                    V.set_conv_precision(prec)
                    try:
                        with torch.no_grad():
                            return f()
                    finally:
                        V.set_conv_precision("f32")
                return run
            methods = {
                "generate(label tensor)": (modules(lambda: G(xc, z, lab)), lambda p: p.generate(xc, z, lab), "generate.blend.cl"),
                "generate(int label 1)": (modules(lambda: G(xc, z, ones)), lambda p: p.generate(xc, z, 1), "generate.c1.cl"),
                "stylize(label tensor)": (modules(lambda: G(xc, E(xs)[0], lab)), lambda p: p.stylize(xc, xs, lab), "stylize.blend.cl"),
                "encode_style": (modules(lambda: E(xs)[0]), lambda p: p.encode_style(xs)[0], "encode.cl"),
                "discriminate": (modules(lambda: D(x, xc, None)[1]), lambda p: p.discriminate(x, xc)[1], "discriminate.cl")}
            for name, (mod, fused, which) in methods.items():
                fns = {"modules": mod, "eager": lambda: fused(eager), "graph": lambda: fused(graph)}
                ref = mod()
                err = {k: float((fns[k]() - ref).abs().max() / ref.abs().max()) for k in ("eager", "graph")}
                n = {k: calls_for(f, a.window) for k, f in fns.items()}
                times = {k: [] for k in fns}
                for _ in range(a.rounds):
                    for k, f in fns.items():        # alternated: every round times each row once
                        times[k].append(window(f, n[k]))
                row = {"net": f"({S}, {Z})", "method": name, "input": f"{B}x3x{S}x{S}", "precision": prec,
                       "fused_launches": len([c for p in eager._plans[which] for c in p.calls]), "max_rel_diff_vs_modules": err}
                for k in fns:
                    ms = [t * 1e3 for t in times[k]]
                    row[k] = {"ms_per_call": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
                              "calls_per_window": n[k], "windows": a.rounds}
                row["modules_over_eager"] = round(row["modules"]["ms_per_call"] / row["eager"]["ms_per_call"], 3)
                row["modules_over_graph"] = round(row["modules"]["ms_per_call"] / row["graph"]["ms_per_call"], 3)
                rows_out.append(row)
            del eager, graph
        del G, E, D
        torch.cuda.empty_cache()
    out = {"metric": "ms per call (network_Style_GAN inference under torch.no_grad())", "unit": "ms",
           "device": torch.cuda.get_device_name(0), "rows": rows_out,
           "method": "one process, rows alternated per round, host clock around a window of calls that ends in a device synchronise; "
                     "median window, spread = min / max over the windows"}
    if a.pieces:
        out["metric"] = "us per call: each new kernel / the fold next to the launches it replaces"
        out["method"] = f"a device event pair around {a.reps} back-to-back calls, the two alternated over {a.rounds} rounds; median, min / max"
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
