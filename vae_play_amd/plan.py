"""Plan-building code shared by the fused plans (engine.FusedVAEStep, engine_gan.FusedVAEGANStep, infer.FusedVAEInference).

A fused step is a fixed list of HIP launches built once for a (model, batch size) pair and replayed every step:
  * ``_Plan``: the launch list and its runner (the per-step host path), with side-stream launches, waits and named hooks;
  * ``_SideCtx``: the side stream the weight gradients run on underneath the main chain;
  * ``PlanBuilder``: the vocabulary the plans are stated in -- buffers, weight packs, BatchNorm, dense layers, column
    sums, 5x5 weight gradients with their CU budget, side slots and the rotation of the split gradient planes.
The sentences written in that vocabulary -- stem, stride-2 blocks, encoder head, decoder trunk, final convolution -- are in sections.py.
"""
from __future__ import annotations

import weakref
from ctypes import c_void_p
from typing import Dict, List, Optional

import torch

from . import _lib, ops

_ACT_RELU, _ACT_NONE = ops.ACT_RELU, ops.ACT_NONE


class _Plan:
    """A list of (c_function, argument list) with the stream slot patched at run time.
    ``flops`` is the algorithmic FLOP count of a call (0 for bandwidth-bound glue); ``timers`` lets
    bench.py bracket selected calls with HIP events on the launch stream.

    A call added with ``side=k`` runs on the side stream (after everything enqueued on the main stream so far) and
    records side event k when it is done; ``wait_side(k)`` makes the main stream wait for that event.  Used to run
    the weight-gradient GEMMs underneath the HBM-bound BatchNorm backward kernels of the next layer."""

    def __init__(self):
        self.calls: List[list] = []

    def add(self, name: str, *args, flops: float = 0.0, tag: str = "", side: Optional[int] = None, side_args: Optional[dict] = None):
        """``side_args`` = {argument index: (value on the main stream, value on the side stream)}: arguments that depend on where
        the call ends up at run time (the weight gradients' CU budget: the whole chip alone, part of it beside the main stream)."""
        fn = getattr(_lib.load(), name)
        a = list(args) + [None]  # last argument of every entry point is the stream
        self.calls.append([name, fn, a, len(a) - 1, flops, tag, side, side_args])

    def add_first(self, name: str, *args, side: Optional[int] = None):
        fn = getattr(_lib.load(), name)
        a = list(args) + [None]
        self.calls.insert(0, [name, fn, a, len(a) - 1, 0.0, "", side, None])

    def wait_side(self, k: int):
        self.calls.append(["__wait_side__", None, [k], 0, 0.0, "", None, None])

    def hook(self, key: str, replaces_next: bool = False):
        """A named point of the plan: ``run(..., hooks={key: fn})`` calls ``fn(side)`` there (between two launches).  With
        ``replaces_next`` the hook stands in for the launch that follows it: that launch runs only when no hook is given."""
        self.calls.append(["__hook__", None, [key, replaces_next], 0, 0.0, "", None, None])

    def run(self, stream_ptr: int, timers: Optional[dict] = None, side: Optional["_SideCtx"] = None, hooks: Optional[dict] = None):
        """``side`` = a ``_SideCtx`` or None (everything on the main stream)."""
        s = c_void_p(stream_ptr)
        it = iter(enumerate(self.calls))
        for ci, (name, fn, a, slot, flops, tag, sev, sargs) in it:
            if fn is None:
                if name == "__hook__":
                    if hooks is not None and a[0] in hooks:
                        hooks[a[0]](side)
                        if a[1]:
                            next(it)
                elif side is not None:                       # main stream waits for a side event
                    torch.cuda.current_stream().wait_event(side.events[a[0]])
                continue
            on_side = side is not None and sev is not None
            if sargs is not None:
                for idx, (v_main, v_side) in sargs.items():
                    a[idx] = v_side if on_side else v_main
            if on_side:
                a[slot] = c_void_p(side.stream.cuda_stream)
                side.launch(name, fn, a, sev)
                continue
            a[slot] = s
            timed = timers is not None and name in timers["names"]
            if timed:
                pool = timers.get("pool")
                if pool is not None:      # events are created once per (instrumented-step slot, call) and re-recorded
                    key = (id(self), ci, timers.get("slot", 0))
                    if key not in pool:
                        pool[key] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    e0, e1 = pool[key]
                else:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            rc = fn(*a)
            if timed:
                e1.record()
                timers["events"].append((name, tag, flops, e0, e1))
            if rc != 0:
                _lib.check(rc, name)


class _SideCtx:
    """Side stream of a fused plan, one event per side launch and the fork event.

    Every side launch forks: the side stream waits for the main stream's work so far (a fork costs the MAIN stream ~6 us: the
    kernel behind the record starts that much later).  Handing several side launches over behind one fork was measured SLOWER
    (3.756 ms at 1, 3.850 at 2, 3.825 at 3, 3.811 at 4; profiles/r02_notes.md section 7): a weight gradient that starts one layer
    late no longer runs underneath the next layer's HBM-bound BatchNorm backward but underneath its MFMA-bound input gradient."""

    def __init__(self, n_events: int):
        self.stream = torch.cuda.Stream()
        self.events = [torch.cuda.Event() for _ in range(n_events)]
        self.fork = torch.cuda.Event()

    def launch(self, name, fn, args, k: int):
        self.fork.record()
        self.stream.wait_event(self.fork)
        rc = fn(*args)
        self.events[k].record(self.stream)
        if rc != 0:
            _lib.check(rc, name)

    def run(self, fn):
        """Fork and call ``fn()`` with the side stream current (Python work that enqueues kernels: optimiser updates, collectives)."""
        self.fork.record()
        self.stream.wait_event(self.fork)
        with torch.cuda.stream(self.stream):
            fn()

    def join(self):
        torch.cuda.current_stream().wait_stream(self.stream)


def _ptr(t):
    """launch argument of a tensor (None: a null pointer; an address computed by the caller passes through)"""
    return t if t is None or isinstance(t, c_void_p) else c_void_p(t.data_ptr())


def side_ctx(step, enabled: bool = True) -> Optional[_SideCtx]:
    """The step's side stream (created on first use), or None when its plan has no side launches or they are switched off."""
    if not step._n_side_events or not enabled:
        return None
    if getattr(step, "_side", None) is None:
        step._side = _SideCtx(step._n_side_events)
    return step._side


def plan_device(module: torch.nn.Module, what: str, plan_only: bool) -> torch.device:
    """Device of the model; ``plan_only`` lets a plan be built over host tensors (structural tests: it is never run)."""
    dev = next(module.parameters()).device
    if dev.type != "cuda" and not plan_only:
        raise _lib.VaePlayHipError(f"{what} needs the model on the HIP device")
    return dev


def sync_counters_on_state_dict(step, module: torch.nn.Module):
    """BatchNorm ``num_batches_tracked`` is advanced lazily (``step.sync_counters()``): make every state_dict() / checkpoint of
    ``module`` see the true counters."""
    me = weakref.ref(step)

    def _sync(mod, prefix, keep_vars):
        o = me()
        if o is not None:
            o.sync_counters()
    return module.register_state_dict_pre_hook(_sync)


def grad_of(p: torch.nn.Parameter) -> torch.Tensor:
    arena = getattr(p, "_vp_arena", None)
    if arena is None:
        raise _lib.VaePlayHipError("parameter has no arena gradient; build the optimiser first")
    return arena.grad_view(p)        # (not p.grad: optimizer.zero_grad(set_to_none=True) drops that attribute, not the slice)


# 5x5 convolution entry points by (arithmetic, BatchNorm statistics from the epilogue): (gather / Conv2d, scatter / ConvTranspose2d)
_CONV5 = {
    ("f32", False): ("vp_conv5_gather_f32", "vp_conv5_scatter_f32"),
    ("f32", True): ("vp_conv5_gather_stats_f32", "vp_conv5_scatter_stats_f32"),
    ("bf16x3", False): ("vp_conv5_gather_bf16x3", "vp_conv5_scatter_bf16x3"),
    ("bf16x3", True): ("vp_conv5_gather_stats_bf16x3", "vp_conv5_scatter_stats_bf16x3"),
    ("f16x2", False): ("vp_conv5_gather_f16", "vp_conv5_scatter_f16"),
    ("f16x2", True): ("vp_conv5_gather_stats_f16", "vp_conv5_scatter_stats_f16"),
    ("f16", False): ("vp_conv5_gather_f16", "vp_conv5_scatter_f16"),       # inference only: no statistics form
}
# workspace query of the statistics epilogue by arithmetic (0: the launch shape cannot emit them)
_CONV5_STATS_WS = {"f32": "vp_conv5_stats_f32_workspace_bytes", "bf16x3": "vp_conv5_stats_workspace_bytes",
                   "f16x2": "vp_conv5_stats_f16_workspace_bytes"}
# fp16 plans: forward layers contract with three products (outputs keep the bf16x3 tolerance), backward layers with two
# (the decoder forward on two products measured 3.51 -> 3.375 ms but 40x the ReLU-mask flips, every forward layer on two
# products puts mu outside the 1e-3 bar: profiles/r02_notes.md section 4)
FWD_PRODUCTS = 3
# "f16" (inference) plans: every 16-bit layer contracts the fp16 hi planes with ONE product
INFER_PRODUCTS = 1
_F16_ARITHS = ("f16x2", "f16")      # arithmetics of the *_f16 entry points (they take products and out_scale)


class PlanBuilder:
    """What the fused plans are built with.  ``precision`` = "f32" | "bf16x3" | "f16x2" (engine.FusedVAEStep documents the
    modes) | "f16" (inference only, infer.FusedVAEInference: fp16 planes contracted with one product); ``side_on``: side-stream launches get side slots (else everything stays on the main stream);
    ``wgrad_cus`` = (main, side) CU budget of the 5x5 weight gradients; ``grad_scale16`` and ``sat`` (the sticky saturation
    flag): the fp16 gradient planes of "f16x2" plans.  Buffers are registered in ``step._bufs``."""

    def __init__(self, step, dev, precision: str, side_on: bool, wgrad_cus, grad_scale16: float = 1.0, sat=None,
                 fuse_stats: bool = True):
        self.lib = _lib.load()
        self.step, self.dev, self.precision = step, dev, precision
        self.x3 = precision in ("bf16x3", "f16x2", "f16")      # 5x5 layers on split 16-bit operands
        self.x2 = precision == "f16x2"
        self.h1 = precision == "f16"                            # one-product fp16 (no gradients: forward / eval sections only)
        self.fp16 = self.x2 or self.h1                          # planes are fp16 (format 1), written by the *_fmt producers
        self.GS = grad_scale16 if self.x2 else 1.0      # scale of gradient planes; 1/GS in the launches that consume them
        self.sat = sat
        self.side_on, self.wgrad_cus, self.fuse_stats = side_on, tuple(wgrad_cus), fuse_stats
        self.bufs: Dict[str, torch.Tensor] = step._bufs
        self.n_side = 0
        self.bn_counts: List[tuple] = []           # (BatchNorm module, forward passes per step)
        self._gemm_calls, self._gemm_need = [], 0
        self._pack_jobs, self._first_pack_jobs = [], []
        # the batched weight re-pack (65 us, ~180 MB of traffic) runs on the side stream, underneath the first
        # encoder block, whose own pack stays on the main stream
        self.k_pack = self.side_slot()

    # ---- buffers ----
    def buf(self, name: str, *shape) -> torch.Tensor:
        t = torch.empty(shape, dtype=torch.float32, device=self.dev)
        assert name not in self.bufs, name
        self.bufs[name] = t
        return t

    def ws(self, name: str, nbytes: int) -> torch.Tensor:
        return self.buf(name, max(4, (int(nbytes) + 3) // 4))

    def sbuf(self, name: str, n: int) -> torch.Tensor:
        """split tensor: (2, n) int16 = hi plane + lo plane (bf16 or fp16 pairs)"""
        t = torch.empty((2, n), dtype=torch.int16, device=self.dev)
        assert name not in self.bufs, name
        self.bufs[name] = t
        return t

    # ---- side stream ----
    def side_slot(self) -> Optional[int]:
        """a new side event for one side-stream launch (None: this plan keeps everything on the main stream)"""
        if not self.side_on:
            return None
        self.n_side += 1
        return self.n_side - 1

    def grad_planes(self, n: int, depth: int = 2):
        """Split output gradients (BatchNorm backward -> 16-bit weight and input gradients) rotate over ``depth`` buffers of n
        elements; before a buffer is rewritten the main stream waits for the side-stream weight gradient that read it.
        (One buffer per layer instead -- the main stream then never waits -- was measured neutral, 3.690 vs 3.691 ms:
        profiles/r02_notes.md section 7.)"""
        self.planes = [self.sbuf(f"g.S{j}", n) for j in range(depth)] if self.x3 else [None] * depth
        self._plane_reader = [None] * depth       # side event of the weight gradient that last read each buffer
        self._plane_turn = 0
        return self.planes

    def next_plane(self, plan: _Plan):
        """(index, buffer) of the next gradient plane of the rotation; pass the index to ``wgrad5`` when a side-stream weight
        gradient reads it"""
        k = self._plane_turn % len(self.planes)
        self._plane_turn += 1
        if self._plane_reader[k] is not None:
            plan.wait_side(self._plane_reader[k])
            self._plane_reader[k] = None
        return k, self.planes[k]

    # ---- weight packs ----
    def pack(self, weight, p0, p1, Cs, Cb, split, Cs_pad=0, first=False, bf16=False):
        """one job of the batched re-pack; split: planes in the plan's format (bf16=True forces bf16 pairs); ``first``: the
        first encoder block's weight, packed on the main stream when the batch runs on the side stream"""
        fmt = (2 if (self.fp16 and not bf16) else 1) if split else 0
        (self._first_pack_jobs if (first and self.k_pack is not None) else self._pack_jobs).append(
            _lib.PackJob(weight.data_ptr(), p0.data_ptr() if p0 is not None else None, p1.data_ptr() if p1 is not None else None,
                         Cs, Cb, Cs_pad, fmt))

    # ---- dense layers: one workspace, sized in finish() (they all run on the main stream) ----
    def _gemm(self, plan, A, sam, sak, Bm, sbn, sbk, C, ldc, bias, M, N, K, mode):
        self._gemm_need = max(self._gemm_need, self.lib.vp_gemm_workspace_bytes(M, N, K))
        plan.add("vp_gemm_f32", A, sam, sak, Bm, sbn, sbk, C, ldc, bias, M, N, K, mode, None, 0)
        self._gemm_calls.append(plan.calls[-1][2])

    def lin_fwd(self, plan, x, W, bias, y, M, N, K):            # y[M,N] = x[M,K] W[N,K]^T + bias
        self._gemm(plan, _ptr(x), K, 1, _ptr(W), K, 1, _ptr(y), N, _ptr(bias), M, N, K, 0)

    def lin_dgrad(self, plan, dy, W, dx, M, N, K):              # dx[M,K] = dy[M,N] W[N,K]
        self._gemm(plan, _ptr(dy), N, 1, _ptr(W), 1, K, _ptr(dx), K, None, M, K, N, 1)

    def lin_wgrad(self, plan, dy, x, dW, M, N, K):              # dW[N,K] = dy[M,N]^T x[M,K]
        self._gemm(plan, _ptr(dy), 1, N, _ptr(x), 1, K, _ptr(dW), K, None, N, K, M, 2)

    def colsum(self, plan, tag, x, out, R, C, side=None):
        """out[C] = column sums of x[R][C]; calls with the same tag share one workspace (they run one after another)"""
        nbytes = self.lib.vp_colsum_workspace_bytes(R, C)
        ws = self.bufs.get(f"{tag}.csws")
        if ws is None:
            ws = self.ws(f"{tag}.csws", nbytes)
        assert ws.numel() * 4 >= nbytes, tag
        plan.add("vp_colsum_f32", _ptr(x), _ptr(out), R, C, _ptr(ws), ws.numel() * 4, side=side)

    # ---- BatchNorm ----
    def bn_fwd(self, plan, tag, x, R, Cn, bn, y, y_s=None, count=1, conv=None):
        """statistics + fused normalise/ReLU of x[R][Cn] (fp32 y and / or split y_s); returns the saved (mean, rstd, workspace).
        Momentum and eps are the module's; ``count`` = forward passes of the module per step (sync_counters).  ``conv`` =
        (family, arithmetic, input, packed weight, geometry, flops): the 5x5 convolution that writes x, emitted here -- when
        its launch shape can emit the statistics from its epilogue the two become ONE call and x is not read again for them.
        Dense layers (R <= 64 rows) take one launch for the whole forward."""
        P = _ptr
        mean, rstd = self.buf(f"{tag}.mean", Cn), self.buf(f"{tag}.rstd", Cn)
        mom, eps = float(bn.momentum), float(bn.eps)
        self.bn_counts.append((bn, count))
        if conv is None and y_s is None and R <= 64 and Cn % 4 == 0:
            # single-launch BatchNorm: statistics + finalisation + normalise/ReLU (-33 us per step, profiles/r02_notes.md section 2)
            plan.add("vp_bn_small_fwd_f32", P(x), R, Cn, eps, mom, P(bn.weight), P(bn.bias), P(mean), P(rstd), P(bn.running_mean),
                     P(bn.running_var), P(y), _ACT_RELU, 0.0)
            return mean, rstd, None
        ws = self.ws(f"{tag}.bnws", self.lib.vp_bn_workspace_bytes(R, Cn))
        fused = conv is not None and self._conv5_fwd(plan, tag, conv, x, bn, eps, mom, mean, rstd)
        if not fused:
            plan.add("vp_bn_stats_f32", P(x), R, Cn, eps, mom, P(mean), P(rstd), P(bn.running_mean), P(bn.running_var),
                     P(ws), ws.numel() * 4)
        if self.x2 and y_s is not None:
            plan.add("vp_bn_act_fwd_split_fmt_f32", P(x), P(mean), P(rstd), P(bn.weight), P(bn.bias), P(y), P(y_s), R, Cn,
                     _ACT_RELU, 0.0, 1)
        else:
            plan.add("vp_bn_act_fwd_split_f32", P(x), P(mean), P(rstd), P(bn.weight), P(bn.bias), P(y), P(y_s), R, Cn, _ACT_RELU, 0.0)
        return mean, rstd, ws

    def _conv5_fwd(self, plan, tag, conv, x, bn, eps, mom, mean, rstd) -> bool:
        """the convolution of bn_fwd; True when it also computed the batch statistics"""
        P = _ptr
        family, arith, a, w, geom, fl = conv
        qgeom = geom if family == 0 else (geom[0], geom[1], geom[2], geom[4], geom[3], geom[5])   # query takes (Cbig, Csmall)
        nst = getattr(self.lib, _CONV5_STATS_WS[arith])(family, *qgeom) if self.fuse_stats else 0
        products = (FWD_PRODUCTS,) if arith == "f16x2" else ()
        name = _CONV5[(arith, bool(nst))][family]
        if nst:
            st = self.ws(f"{tag}.statws", nst)
            plan.add(name, P(a), P(w), P(x), *geom, *products, eps, mom, P(mean), P(rstd), P(bn.running_mean), P(bn.running_var),
                     P(st), st.numel() * 4, flops=fl, tag=f"{tag}.fwd")
            return True
        self.conv5(plan, family, arith, a, w, x, geom, flops=fl, tag=f"{tag}.fwd")
        return False

    def conv5(self, plan, family, arith, a, w, out, geom, products=FWD_PRODUCTS, alpha=1.0, bias=None, act=_ACT_NONE, **kw):
        """5x5 convolution without statistics: family 0 = gather (nn.Conv2d, or a ConvTranspose2d's input gradient; bias and
        activation in the epilogue), 1 = scatter.  "f16x2" and "f16" take the number of fp16 products and the factor the
        accumulators are multiplied by (1/grad_scale16 for gradient planes)."""
        P = _ptr
        name = _CONV5[(arith, False)][family]
        tail = (products, alpha) if arith in _F16_ARITHS else ()
        if family == 0:
            plan.add(name, P(a), P(w), P(bias), P(out), *geom, act, *tail, **kw)
        else:
            plan.add(name, P(a), P(w), P(out), *geom, *tail, **kw)

    # ---- inference: eval-mode BatchNorm as constants ----
    def bn_fold(self, plan, tag, bn):
        """(scale, shift, rstd) of an eval-mode BatchNorm -- s = gamma / sqrt(running_var + eps), t = beta - running_mean s --
        written by one launch of ``plan`` (the plan that runs once per set of weights, not per call)"""
        P = _ptr
        Cn = bn.running_mean.numel()
        scale, shift, rstd = self.buf(f"{tag}.scale", Cn), self.buf(f"{tag}.shift", Cn), self.buf(f"{tag}.rstd", Cn)
        plan.add("vp_bn_fold_f32", P(bn.weight), P(bn.bias), P(bn.running_mean), P(bn.running_var), float(bn.eps), P(scale), P(shift),
                 P(rstd), Cn, tag=f"{tag}.fold")
        return scale, shift, rstd

    def conv5_bn_eval(self, plan, tag, family, arith, a, w, geom, bn, folded, y, y_s=None, flops=0.0, out_fmt=ops.OUT_F16_HI) -> bool:
        """5x5 convolution + eval-mode BatchNorm + ReLU writing fp32 ``y`` and / or split planes ``y_s``: ONE launch with the affine
        epilogue where the library takes the launch shape (returns True), else convolution + one normalise pass over a scratch
        buffer.  ``arith`` = "bf16x3" | "f32" | "f16"; ``geom`` as conv5's; ``folded`` = bn_fold's result.  ``out_fmt`` ("f16"
        only): what the consumer of ``y_s`` reads -- ops.OUT_F16_HI for a one-product layer, ops.OUT_BF16_PAIR for a bf16x3 kernel."""
        P = _ptr
        scale, shift, rstd = folded
        qgeom = geom if family == 0 else (geom[0], geom[1], geom[2], geom[4], geom[3], geom[5])   # query takes (Cbig, Csmall)
        if self.lib.vp_conv5_affine_supported(family, ops.AFFINE_PRECISION[arith], *qgeom):
            name = ("vp_conv5_gather_affine_", "vp_conv5_scatter_affine_")[family] + arith
            tail = (out_fmt,) if arith == "f16" else ()
            plan.add(name, P(a), P(w), P(scale), P(shift), P(y), P(y_s), *geom, _ACT_RELU, *tail, flops=flops, tag=f"{tag}.fwd")
            return True
        Bn, Hs, Ws, stride = geom[0], geom[1], geom[2], geom[5]
        Cout = geom[4]
        R = Bn * Hs * Ws * (stride * stride if family == 1 else 1)
        c = self.buf(f"{tag}.c", R * Cout)
        self.conv5(plan, family, arith, a, w, c, geom, products=INFER_PRODUCTS if arith == "f16" else FWD_PRODUCTS, flops=flops,
                   tag=f"{tag}.fwd")
        self.bn_eval(plan, tag, c, R, Cout, bn, rstd, y, y_s)
        return False

    def bn_eval(self, plan, tag, x, R, Cn, bn, rstd, y, y_s=None):
        """eval-mode BatchNorm + ReLU of x[R][Cn] as its own pass: running mean, folded rstd"""
        P = _ptr
        if y_s is None:
            plan.add("vp_bn_act_fwd_f32", P(x), P(bn.running_mean), P(rstd), P(bn.weight), P(bn.bias), P(y), R, Cn, _ACT_RELU, 0.0,
                     tag=f"{tag}.bn")
        elif self.fp16:
            plan.add("vp_bn_act_fwd_split_fmt_f32", P(x), P(bn.running_mean), P(rstd), P(bn.weight), P(bn.bias), P(y), P(y_s), R, Cn,
                     _ACT_RELU, 0.0, ops.SPLIT_F16, tag=f"{tag}.bn")
        else:
            plan.add("vp_bn_act_fwd_split_f32", P(x), P(bn.running_mean), P(rstd), P(bn.weight), P(bn.bias), P(y), P(y_s), R, Cn,
                     _ACT_RELU, 0.0, tag=f"{tag}.bn")

    def bn_bwd(self, plan, x, dy, dx, R, Cn, bn, saved, dx_s=None, gfn=grad_of):
        """BatchNorm + ReLU backward; writes dx (fp32) and / or dx_s (split planes; fp16 pairs of GS * dx in "f16x2" plans) and
        the module's parameter gradients (``gfn``: where a parameter's gradient lives)"""
        P = _ptr
        mean, rstd, ws = saved
        if dx_s is None and R <= 64 and Cn % 4 == 0:
            plan.add("vp_bn_small_bwd_f32", P(x), P(dy), P(mean), P(rstd), P(bn.weight), P(bn.bias), P(dx), P(gfn(bn.weight)),
                     P(gfn(bn.bias)), R, Cn, _ACT_RELU, 0.0, 1)
        elif self.x2 and dx_s is not None:
            plan.add("vp_bn_act_bwd_split_fmt_sat_f32", P(x), P(dy), P(mean), P(rstd), P(bn.weight), P(bn.bias), P(dx), P(dx_s),
                     P(gfn(bn.weight)), P(gfn(bn.bias)), R, Cn, _ACT_RELU, 0.0, 1, 1, self.GS, P(self.sat), P(ws), ws.numel() * 4)
        else:
            plan.add("vp_bn_act_bwd_split_f32", P(x), P(dy), P(mean), P(rstd), P(bn.weight), P(bn.bias), P(dx), P(dx_s),
                     P(gfn(bn.weight)), P(gfn(bn.bias)), R, Cn, _ACT_RELU, 0.0, 1, P(ws), ws.numel() * 4)

    # ---- 5x5 weight gradients ----
    def wgrad_workspace(self, layers, at_least: int = 0) -> torch.Tensor:
        """one workspace for the 5x5 weight gradients (they run one after another); ``layers`` = (batch, H, Cbig, Csmall) of
        the stride-2 layers.  Its size selects the split depth of the split-operand kernels."""
        n = at_least
        for Bn, Hs, Cbig, Csmall in layers:      # (the split-bf16 query may ask for more: tap pairs split the pixels deeper)
            n = max(n, self.lib.vp_conv5_wgrad_workspace_bytes(Bn, Hs, Hs, Cbig, Csmall, 2),
                    self.lib.vp_conv5_wgrad_bf16x3_workspace_bytes(Bn, Hs, Hs, Cbig, Csmall, 2))
        self.ws_wg = self.ws("g.wgrad.ws", n)
        return self.ws_wg

    def wgrad5(self, plan, big_s, small_s, dw, geom, plane: int, **kw):
        """split-operand 5x5 weight gradient on the side stream; it reads gradient plane ``plane`` (next_plane), which the main
        stream will not rewrite before it is done.  CU budget: ``wgrad_cus`` (main, side), chosen where the call runs."""
        P, ws = _ptr, self.ws_wg
        k = self.side_slot()
        self._plane_reader[plane] = k
        if self.x2:
            plan.add("vp_conv5_wgrad_f16x2_cus", P(big_s), P(small_s), P(dw), *geom, 1.0 / self.GS, 0, P(ws), ws.numel() * 4,
                     side=k, side_args={4 + len(geom): self.wgrad_cus}, **kw)
        else:
            plan.add("vp_conv5_wgrad_bf16x3_cus", P(big_s), P(small_s), P(dw), *geom, 0, P(ws), ws.numel() * 4,
                     side=k, side_args={3 + len(geom): self.wgrad_cus}, **kw)

    # ---- the end of a plan ----
    def dense_workspace(self, prefix: str = ""):
        """the dense layers' workspace alone: the end of a builder that queued no weight pack (``finish`` needs at least one)"""
        wsg = self.ws(f"{prefix}gemm.ws", self._gemm_need)
        for a in self._gemm_calls:
            a[13], a[14] = _ptr(wsg), wsg.numel() * 4

    def finish(self, fwd: _Plan, prefix: str = ""):
        """batched weight re-pack at the head of the forward plan, the dense layers' workspace; sets the step's
        ``_n_side_events``.  ``prefix``: of a builder that extends a finished plan (its workspace's name, its array of pack jobs)"""
        step = self.step
        jobs = (_lib.PackJob * len(self._pack_jobs))(*self._pack_jobs)
        setattr(step, f"_{prefix.replace('.', '_')}pack_jobs", jobs)                 # host array read by every call: keep it alive
        fwd.add_first("vp_pack_w5_batch", jobs, len(self._pack_jobs), side=self.k_pack)
        if self._first_pack_jobs:
            step._pack_jobs0 = (_lib.PackJob * len(self._first_pack_jobs))(*self._first_pack_jobs)
            fwd.add_first("vp_pack_w5_batch", step._pack_jobs0, len(self._first_pack_jobs))
        wsg = self.ws(f"{prefix}gemm.ws", self._gemm_need)
        for a in self._gemm_calls:
            a[13], a[14] = _ptr(wsg), wsg.numel() * 4
        step._n_side_events = self.n_side
