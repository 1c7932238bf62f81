#!/usr/bin/env python3
"""bench.py -- images/sec of the full VAE training step (fwd + BCE/KL loss + bwd + gradient
all-reduce + Adam) on N MI355X GPUs, one process per GPU.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json config 3): 128x128x3 images, latent 128, 32 images per GPU
(global batch 256 at 8 GPUs -> weak scaling), synthetic uniform[0,1) pixels, random-init weights
(VaeGan.init_parameters rule, seed 0), Adam(lr=1e-4).  Headline arithmetic (`dtype`): "bf16x3" = every 5x5
contraction as three bf16 MFMAs on split-bf16 (hi + lo) operands with fp32 accumulation (16 significant bits per
operand, ~1e-5 parity with the fp32 reference); `--precision f32` runs every contraction on the exact-fp32 MFMA
(v_mfma_f32_32x32x2_f32).  Prints ONE JSON line on rank 0.  `roofline` is for the dominant kernel family of the
step (the 5x5 implicit-GEMM convolutions, MFMA-bound): algorithmic FLOPs of its launches / their summed HIP-event
durations inside the timed region.  `variants` (one GPU only, measured after the headline's timed region, same
protocol): the exact-f32 mode, the f16x2 mode (fp16 pairs: three MFMAs per product forward, two backward), per-GPU batches
64 / 128 / 256 and BASELINE config 2 (64x64x3, z=64, batch 128).  `comm` says what the gradient exchange ran on.
`cpu_baseline` times the CPU oracle (oracle/ref_cpu.py = the reference's torch-CPU algorithm) on this box's host cores: 2 warm-ups,
best of 5, threads = min(affinity mask, cgroup CPU quota).

A plain run measures the headline only: set-up, W warm-up steps (plus the untimed settle steps), exactly K timed steps of the
uninstrumented step, one JSON line.  `--full` adds everything else, as described above: the roofline events (one instrumented step
inside the timed region, serial schedule), the per-bucket `comm` trace on several ranks, `--tags-out`, the `variants` /
`exact_f32` legs and `cpu_baseline`.

`--dump-outputs DIR` writes, after the timed region, what the last timed step computed, as float32 .npy files: loss.npy,
recon.npy, kl.npy (the step's return values), x_tilde.npy, mu.npy, logvar.npy, param.<name>.npy (every parameter after the
update) and buffer.<name>.npy (BatchNorm running statistics).  An array larger than its cap is replaced by a fixed, seeded sample
of its elements (sorted flat positions); the whole set stays under 64 MB.  Inputs and initial weights are seeded, so two builds
run with the same arguments can be compared file for file, e.g.

    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs bench_out/
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

# algorithmic GFLOP per image for one training step (fwd + dgrad + wgrad, transposed
# convs without zero insertion)
STEP_GFLOP = {32: 0.6141, 64: 4.0301, 128: 22.2088, 256: 112.0225}
PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA (v_mfma_f32_32x32x16_bf16)
CONV_CALLS = {"vp_conv5_gather_f32", "vp_conv5_scatter_f32", "vp_conv5_wgrad_f32", "vp_conv5_gather_stats_bf16x3", "vp_conv5_scatter_stats_bf16x3",
              "vp_conv5_gather_bf16x3", "vp_conv5_scatter_bf16x3", "vp_conv5_wgrad_bf16x3",
              "vp_conv_gather_bf16x3", "vp_conv_wgrad_bf16x3",
              "vp_conv5_smallin_dgrad_bf16x3", "vp_conv5_smallout_bf16x3", "vp_conv5_smallout_wgrad_bf16x3", "vp_conv5_gather_f16", "vp_conv5_scatter_f16", "vp_conv5_wgrad_f16x2", "vp_conv5_gather_stats_f16",
              "vp_conv5_scatter_stats_f16", "vp_conv_gather_f16", "vp_conv_wgrad_f16x2",
              "vp_conv5_wgrad_bf16x3_cus", "vp_conv5_wgrad_f16x2_cus", "vp_conv5_wgrad_f32_cus",
              "vp_conv5_gather_stats_f32", "vp_conv5_scatter_stats_f32", "vp_conv5_smallin_dgrad_f32", "vp_conv5_smallout_wgrad_f32",
              "vp_conv_gather_f32", "vp_conv_wgrad_f32"}


def mfma_products(name, tag):
    """MFMAs issued per algorithmic product by the launch `name` (tag = its layer): 3 on bf16 pairs, 3 (forward layers) or 2
    (backward layers) on fp16 pairs, 1 on the exact-fp32 kernels."""
    name = name.replace("_cus", "")      # (the weight gradients' entry points with a CU budget: same kernels)
    if name.endswith("bf16x3"):
        return 3
    if name.endswith("_f16x2"):
        return 2
    if name.endswith("_f16"):
        return 3 if (tag or "").endswith(".fwd") else 2
    return 1


def measured_traffic(api_name):
    """HBM bytes per launch of a conv family from the committed PMC passes (profiles/*_traffic.json, newest round);
    None when no measurement is on file for that kernel."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_traffic.json")))
    if not files:
        return None, None
    with open(files[-1]) as f:
        d = json.load(f)
    return d.get(api_name), os.path.basename(files[-1])


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--img", type=int, default=128)
    ap.add_argument("--z", type=int, default=128)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--batch-per-gpu", type=int, default=32)
    ap.add_argument("--graph", action="store_true", help="replay the step from a captured hipGraph "
                    "(roofline events are then taken in a separate instrumented pass)")
    ap.add_argument("--precision", choices=["bf16x3", "f32", "f16x2"], default="bf16x3",
                    help="bf16x3: split-bf16 MFMA (3 bf16 MFMAs per product, fp32 accumulate, ~1e-5 parity); "
                         "f32: exact fp32 MFMA")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-steps", type=int, default=5, help="timed CPU-oracle steps (best is reported) after 2 warm-ups")
    ap.add_argument("--no-variants", action="store_true", help="skip the f32 / batch-sweep / config-2 variant measurements")
    ap.add_argument("--variant-steps", type=int, default=20)
    ap.add_argument("--dp-factored", type=int, choices=[0, 1], default=None,
                    help="multi-GPU: 1 = exchange the two factors of encoder.fc.0's weight gradient (all-gather) instead of "
                         "all-reducing the 134 MB product; default: the engine's (VP_DP_FACTORED, on)")
    ap.add_argument("--dp-enc-tail", type=int, choices=[0, 1], default=None,
                    help="multi-GPU: 1 = reduce the deep encoder blocks' conv gradients in their own early bucket")
    ap.add_argument("--dp-overlap", type=int, choices=[0, 1], default=1,
                    help="multi-GPU: 0 = ONE all-reduce of the whole gradient arena after backward")
    ap.add_argument("--no-settle", action="store_true", help="do exactly --warmup untimed steps (no power-state settling)")
    ap.add_argument("--tags-out", type=str, default="", help="write per-layer conv timings (JSON) to this file (needs --full)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline events, comm trace, variants, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="write what the last timed step computed to DIR/<name>.npy (float32, at most 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.tags_out and not args.full:
        ap.error("--tags-out needs --full (the per-layer timings come from the instrumented step)")
    return args


def cpu_baseline(args):
    """The oracle (= reference algorithm on torch CPU) on the host cores: bounded sample.
    Protocol of BASELINE.md section 4 / SURVEY.md 8d: every core this process may use, 2 warm-up steps, best of 5."""
    from oracle import ref_cpu as O
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    # the CPU share this process really has: the affinity mask of a shared GPU box names all 256 hardware threads while the
    # container's cgroup quota is 16 CPUs -- 256 torch threads on a 16-CPU quota measured 1.0 images/s (oversubscription)
    # against 35 with 16.  threads = min(affinity, cgroup quota); both are reported.
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            if q != "max":
                quota = max(1, int(float(q) / float(per) + 0.5))
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                q, per = int(f.read()), int(g.read())
                if q > 0:
                    quota = max(1, int(q / per + 0.5))
        except (OSError, ValueError):
            pass
    threads = int(os.environ.get("VAEPLAY_CPU_THREADS", min(avail, quota) if quota else avail))
    torch.set_num_threads(threads)
    B, C, S, z = args.batch_per_gpu, args.channels, args.img, args.z
    L = O.iter_level_for(S)
    p = O.init_params(C, z, L, seed=0)
    O.require_grad(p)
    opt = O.make_optimizer(p, "adam", 1e-4)
    x, eps = O.synthetic_batch(B, C, S, z)
    t_w = time.perf_counter()
    for _ in range(2):
        O.train_step(p, opt, x, eps, L)  # warm-up
        if time.perf_counter() - t_w > 30.0:
            break
    best = float("inf")
    t_all = time.perf_counter()
    done = 0
    for _ in range(args.cpu_steps):
        t0 = time.perf_counter()
        O.train_step(p, opt, x, eps, L)
        best = min(best, time.perf_counter() - t0)
        done += 1
        if time.perf_counter() - t_all > 40.0:      # bounded sample: the default run must finish within minutes
            break
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"value": round(B / best, 2), "unit": "images/sec", "cores": threads, "threads": threads,
            "host_cores": os.cpu_count(), "affinity_cores": avail, "cgroup_cpus": quota, "cpu_model": model, "kind": "port",
            "sample": f"best of {done} timed steps after 2 warm-ups, batch {B}, {S}x{S}x{C}, z={z}, "
                      f"torch {torch.__version__} CPU fp32, {threads} threads = min(affinity mask, cgroup CPU quota) of this box"}


SETTLE_STEPS = 200


def build_step(B, S, C, z, precision, rank, graph=False):
    """Model + optimiser + fused plan + resident synthetic batch for one workload."""
    import vae_play_amd as V
    from vae_play_amd import engine, optim, parallel
    torch.manual_seed(0)
    vae = V.VAE(S, z, C, init_rule=True).to("cuda").train()     # same seed on every rank = replicated weights
    opt = optim.Adam(vae.parameters(), lr=1e-4)
    parallel.broadcast_flat_params(opt.flat_param, 0)
    fused = engine.FusedVAEStep(vae, opt, B, S, C, precision=precision)
    gx = torch.Generator().manual_seed(1234 + rank)
    ge = torch.Generator().manual_seed(4321 + rank)
    x = torch.rand(B, C, S, S, generator=gx).cuda()               # inputs resident in HBM before timing
    eps = torch.randn(B, z, generator=ge).cuda()
    if graph:
        fused.capture()
    return fused, x, eps


def measure(fused, x, eps, steps, untimed, world, graph, overlap=True, tags_out="", instrument=True, snapshot=None):
    """`untimed` warm-up/settle steps, then EXACTLY `steps` timed steps between barrier + synchronize pairs.
    HIP events bracket the convolution launches of ONE timed step only (the middle one), with pre-created events: an event
    record is a barrier packet on the stream and 52 of them per step cost 0.4-2 ms of pipeline bubbles, which made the figure
    depend on how many steps were instrumented.  The instrumented step also runs the SERIAL schedule (weight gradients on the
    main stream instead of the side stream, optimiser at the end) so that an event pair times one kernel alone: it costs
    ~0.6 ms more than a plain step, i.e. +0.03 ms on the 20-step average (two instrumented steps, rounds 1-3: +0.06 ms = 1.7 % --
    the same binary over 1 500 steps measures 3.43 ms where the 20-step region with two of them measured 3.49); the other K-1
    steps run the concurrent schedule.  ``instrument=False`` (a plain run of bench.py): no events, no instrumented step, all K
    timed steps are the plain step.  ``snapshot(loss, recon, kl)`` is called once right after the timed region, before anything
    else can overwrite the plan's output buffers; its result is returned as ``outputs``."""
    for _ in range(untimed):
        fused.step(x, eps, overlap=overlap)
    timers = None if (graph or not instrument) else {"names": CONV_CALLS, "events": [], "pool": {}, "slot": 0}
    N_INST = 1
    if timers is not None:    # create the events (hipEventCreate is not free) outside the timed region
        for sl in range(N_INST):
            timers["slot"] = sl
            fused.step(x, eps, timers, overlap=overlap)
        torch.cuda.synchronize()
        timers["events"].clear()

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    inst = [steps // 2] if timers is not None else []
    trace = None
    if world > 1 and timers is not None:      # several ranks: the instrumented steps also trace their collectives (comm.buckets)
        from vae_play_amd import parallel
        trace = parallel.CommTrace()
    barrier()
    t0 = time.perf_counter()
    for i in range(steps):
        if i in inst:
            timers["slot"] = inst.index(i)
            loss, recon, kl = fused.step(x, eps, timers, overlap=overlap, comm_trace=trace)
        else:
            loss, recon, kl = fused.step(x, eps, None, overlap=overlap)
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = tmax.item()
    final_loss = loss.item()
    outputs = snapshot(loss, recon, kl) if snapshot is not None else None
    measured = "timed-region" if instrument else None
    if timers is None and instrument:  # graph replay cannot carry events: instrumented eager pass of the same K steps
        timers = {"names": CONV_CALLS, "events": []}
        for _ in range(steps):
            fused.forward_backward(x, eps, timers)
        torch.cuda.synchronize()
        measured = "instrumented-pass-after-timed-region"
    fam = {}
    for name, tag, flops, e0, e1 in (timers["events"] if timers is not None else []):
        d = fam.setdefault(name.replace("_stats_", "_").replace("_cus", ""), [0.0, 0.0, 0, 0.0])
        d[0] += flops
        d[1] += e0.elapsed_time(e1) * 1e-3
        d[2] += 1
        d[3] += flops * mfma_products(name, tag)
    if tags_out:
        per = {}
        for name, tag, flops, e0, e1 in timers["events"]:
            d = per.setdefault(tag, [0.0, 0.0, 0])
            d[0] += flops; d[1] += e0.elapsed_time(e1) * 1e-3; d[2] += 1
        with open(tags_out, "w") as f:
            json.dump({k: {"ms": round(v[1] / v[2] * 1e3, 4), "gflop": round(v[0] / v[2] / 1e9, 3),
                           "tflops": round(v[0] / v[1] / 1e12, 2)} for k, v in per.items()}, f, indent=1)
    n_inst = len(inst) if measured == "timed-region" else steps if instrument else 0
    return {"elapsed": elapsed, "loss": final_loss, "fam": fam, "n_inst": n_inst, "measured": measured,
            "comm_trace": trace.summary() if trace is not None else None, "outputs": outputs}


DUMP_CAP_OUTPUT = 1 << 22     # elements kept of x_tilde / mu / logvar (16 MB each at most)
DUMP_CAP_PARAM = 1 << 17      # elements kept of one parameter or buffer (512 KB)
DUMP_MAX_BYTES = 64 << 20


def _sample(t, cap, seed):
    """``t`` flattened, whole when it has at most ``cap`` elements, else a fixed sample of ``cap`` of them: positions drawn without
    replacement by a generator seeded with ``seed``, in increasing order."""
    import numpy as np
    flat = t.detach().reshape(-1)
    if flat.numel() > cap:
        pos = np.sort(np.random.default_rng(seed).choice(flat.numel(), cap, replace=False))
        flat = flat[torch.from_numpy(pos).to(flat.device)]
    return flat.float().cpu().numpy()


def output_snapshot(fused):
    """What one call of ``fused.step`` hands its caller, copied to the host: the returned (loss, recon, kl), the plan's forward
    outputs (x_tilde, mu, logvar) and the model state the step updated (parameters, BatchNorm running statistics).  Float32; an
    array above its cap is a seeded sample (``_sample``), so the set is the same from run to run for the same arguments."""
    def snap(loss, recon, kl):         # (called after the timed region's closing synchronize)
        out = {"loss": loss, "recon": recon, "kl": kl}
        out = {k: v.detach().float().cpu().numpy().reshape(()) for k, v in out.items()}
        for i, (k, v) in enumerate((("x_tilde", fused.x_tilde), ("mu", fused.mu), ("logvar", fused.logvar))):
            out[k] = (v.detach().float().cpu().numpy() if v.numel() <= DUMP_CAP_OUTPUT else _sample(v, DUMP_CAP_OUTPUT, 100 + i))
        for i, (k, p) in enumerate(fused.vae.named_parameters()):
            out["param." + k] = p.detach().float().cpu().numpy() if p.numel() <= DUMP_CAP_PARAM else _sample(p, DUMP_CAP_PARAM, 1000 + i)
        for i, (k, b) in enumerate(fused.vae.named_buffers()):
            if b.is_floating_point():
                out["buffer." + k] = _sample(b, DUMP_CAP_PARAM, 2000 + i)
        return out
    return snap


def write_outputs(outputs, out_dir):
    import numpy as np
    total = sum(a.nbytes for a in outputs.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes of outputs exceed the {DUMP_MAX_BYTES}-byte budget")
    os.makedirs(out_dir, exist_ok=True)
    for k, a in outputs.items():
        np.save(os.path.join(out_dir, k + ".npy"), np.asarray(a, dtype=np.float32))


def roofline_of(m, steps, B, S, C, z):
    fam = m["fam"]
    dom = max(fam, key=lambda k: fam[k][1])
    tot_f = sum(v[0] for v in fam.values())
    tot_t = sum(v[1] for v in fam.values())
    ach = fam[dom][0] / fam[dom][1] / 1e12
    is16 = dom.endswith("bf16x3") or dom.endswith("f16x2") or dom.endswith("_f16")
    per_product = fam[dom][3] / fam[dom][0]      # MFMAs per product, averaged over the family's launches (fp16: 3 forward, 2 backward)
    peak = PEAK_BF16_MFMA_TFLOPS if is16 else PEAK_FP32_MFMA_TFLOPS       # fp16 and bf16 MFMAs have the same dense peak
    kern = "wgrad5_kernel (one kernel row of 5 taps per workgroup) + slab reduction" if "wgrad" in dom else "igemm16_kernel"
    kdesc = (f"{kern}, 3 x v_mfma_f32_32x32x16_bf16 per product" if dom.endswith("bf16x3")
             else f"{kern}, 2 (backward) or 3 (forward) x v_mfma_f32_32x32x16_f16 per product" if is16
             else ("wgrad5f_kernel (rows of taps) + slab reduction" if "wgrad" in dom else "igemm16_kernel in fp32 mode") + ", v_mfma_f32_32x32x2_f32")
    # the committed PMC passes were taken on the default workload only
    traffic, traffic_src = measured_traffic(dom) if (S, C, z, B) == (128, 3, 128, 32) else (None, None)
    return {"bound": "mfma", "kernel": f"{dom} ({kdesc})",
            "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s",
            "frac": round(ach / peak, 4), "traffic": traffic, "traffic_unit": "HBM-side bytes per launch (PMC)",
            "traffic_source": traffic_src,
            "mfma_issue_frac": round(ach * per_product / peak, 4), "mfma_per_product": round(per_product, 3),
            "launches": fam[dom][2], "avg_launch_ms": round(fam[dom][1] / fam[dom][2] * 1e3, 4),
            "all_conv_families_tflops": round(tot_f / tot_t / 1e12, 2),
            "conv_share_of_step_time": round(tot_t / m["n_inst"] / (m["elapsed"] / steps), 3),
            "instrumented_steps": m["n_inst"],
            "measured": m["measured"]}


def comm_record(world, args, trace=None):
    """What the gradient exchange ran on (so that a multi-GPU line can be checked from the JSON alone).  Several ranks: ``buckets``
    = every collective of a step with its bytes and its device time (issue-ready -> result-ready on a communicator-side stream,
    queueing behind earlier buckets included), ``exposed_ms_per_step`` = the time rank 0's main stream spent waiting for
    collectives, both from the instrumented steps of the timed region (serial kernel schedule, like the roofline events)."""
    rec = {"backend": None, "world_size_seen": 1, "rccl_version": None, "exchange": "none (one rank)"}
    try:
        v = torch.cuda.nccl.version()
        rec["rccl_version"] = ".".join(str(i) for i in v) if isinstance(v, (tuple, list)) else str(v)
    except Exception:
        pass
    if world > 1 and dist.is_initialized():
        rec["backend"] = dist.get_backend()
        rec["world_size_seen"] = dist.get_world_size()
        factored = os.environ.get("VP_DP_FACTORED", "1") != "0"
        tail = os.environ.get("VP_DP_ENC_TAIL", "1") != "0"
        if not args.dp_overlap:
            rec["exchange"] = "one SUM all-reduce of the flat gradient arena after backward"
        else:
            rec["exchange"] = ("bucketed SUM all-reduce of the flat gradient arena underneath backward (decoder | encoder dense | "
                               + ("deep encoder convs | " if tail else "") + "rest)"
                               + ("; encoder.fc.0 weight gradient exchanged as its two factors (2 all-gathers) and contracted locally"
                                  if factored else ""))
        rec["dp_factored"], rec["dp_enc_tail"], rec["dp_overlap"] = factored, tail, bool(args.dp_overlap)
        if trace is not None:
            rec.update(trace)
            n_ar = trace["collectives_per_step"].get("all_reduce", 0)
            rec["all_reduces_per_step"] = n_ar
            rec["all_gathers_per_step"] = trace["collectives_per_step"].get("all_gather", 0)
    return rec


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback exists for the product path)")
    torch.cuda.set_device(local if local < torch.cuda.device_count() else 0)
    if args.dp_factored is not None:
        os.environ["VP_DP_FACTORED"] = str(args.dp_factored)
    if args.dp_enc_tail is not None:
        os.environ["VP_DP_ENC_TAIL"] = str(args.dp_enc_tail)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("VP_BENCH_BACKEND", "nccl")     # "gloo": rehearsal of the multi-rank path on one GPU
        if backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend, rank=rank, world_size=world)

    B, C, S, z = args.batch_per_gpu, args.channels, args.img, args.z
    fused, x, eps = build_step(B, S, C, z, args.precision, rank, args.graph)

    # W untimed warm-up steps, then untimed "settle" steps up to SETTLE_STEPS in total: a fresh process starts with the
    # GPU in a low power state and a 0.2-s timed region taken right after a short warm-up measured 4.8-6.6 ms/step
    # for the same binary; after ~1 s of load successive runs agree within 4 % (profiles/r01_c_notes.md).
    # The count is fixed (not time-based) so that every rank of a multi-GPU run executes the same collectives.
    n_settle = max(0, SETTLE_STEPS - args.warmup) if not args.no_settle else 0
    m = measure(fused, x, eps, args.steps, args.warmup + n_settle, world, args.graph, overlap=bool(args.dp_overlap),
                tags_out=args.tags_out if rank == 0 else "", instrument=args.full,
                snapshot=output_snapshot(fused) if args.dump_outputs and rank == 0 else None)
    if m["outputs"] is not None:
        write_outputs(m["outputs"], args.dump_outputs)

    out = None
    if rank == 0:
        ips = world * B * args.steps / m["elapsed"]
        out = {
            "metric": f"images/sec (train step, {S}x{S} VAE)", "value": round(ips, 1), "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "settle_steps": n_settle,
            "ms_per_step": round(m["elapsed"] / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
            "config": {"workload": f"networks VAE {S}x{S}x{C} latent={z} train step (fwd+BCE/KL+bwd+allreduce+Adam), "
                                   f"{B} images/GPU, global batch {B * world}", "parallelism": f"dp{world}",
                       "per_gpu_batch": B, "global_batch": B * world, "graph": bool(args.graph),
                       "precision": args.precision},
            "images_per_sec_per_gpu": round(ips / world, 1),
            "step_algorithmic_tflops_per_gpu": round(ips / world * STEP_GFLOP.get(S, 0.0) / 1e3, 1),
            "loss": round(m["loss"], 4),
            **({"roofline": roofline_of(m, args.steps, B, S, C, z)} if args.full else {}),
            "comm": comm_record(world, args, m.get("comm_trace")),
        }
    # ---- variants: one GPU only (their collectives would have to match on every rank), after the headline ----------------
    if world == 1 and args.full and not args.no_variants:
        del fused
        torch.cuda.empty_cache()
        todo = []
        if args.precision != "f32":
            todo.append(("f32", B, S, C, z))
        if args.precision != "f16x2":      # the cheaper contraction mode (declared tolerance 1e-3 on outputs, tests/test_gpu_f16x2.py)
            todo.append(("f16x2", B, S, C, z))
        for b2 in (64, 128, 256):
            if b2 != B:
                todo.append((args.precision, b2, S, C, z))
        if (S, C, z, B) != (64, 3, 64, 128):
            todo.append((args.precision, 128, 64, 3, 64))              # BASELINE.json config 2
        variants = []
        for prec, b2, s2, c2, z2 in todo:
            try:
                f2, x2, e2 = build_step(b2, s2, c2, z2, prec, rank)
                m2 = measure(f2, x2, e2, args.variant_steps, 30, 1, False)
                ips2 = b2 * args.variant_steps / m2["elapsed"]
                variants.append({
                    "workload": f"{s2}x{s2}x{c2} z{z2} B{b2}", "precision": prec, "batch_per_gpu": b2,
                    "steps": args.variant_steps, "ms_per_step": round(m2["elapsed"] / args.variant_steps * 1e3, 4),
                    "images_per_sec": round(ips2, 1),
                    "step_algorithmic_tflops": round(ips2 * STEP_GFLOP.get(s2, 0.0) / 1e3, 1),
                    "roofline": roofline_of(m2, args.variant_steps, b2, s2, c2, z2)})
                del f2, x2, e2
                torch.cuda.empty_cache()
            except Exception as ex:          # a variant must never take the headline line down with it
                variants.append({"workload": f"{s2}x{s2}x{c2} z{z2} B{b2}", "precision": prec, "error": repr(ex)[:200]})
        out["variants"] = variants
        # the reference-width leg at top level: the like-for-like figure against the reference's fp32 arithmetic
        for v in variants:
            if v.get("precision") == "f32" and v.get("batch_per_gpu") == B and "error" not in v and v["workload"].startswith(f"{S}x{S}x{C} "):
                out["exact_f32"] = {"ms_per_step": v["ms_per_step"], "images_per_sec": v["images_per_sec"],
                                    "step_algorithmic_tflops": v["step_algorithmic_tflops"], "roofline": v["roofline"],
                                    "dtype": "f32 (v_mfma_f32_32x32x2_f32 / 16x16x4: exact fp32 products, fp32 accumulate)"}
                break
    if rank == 0:
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
