"""Fused VAE training step: the whole forward + loss + backward of SURVEY.md 3.3 as a fixed,
pre-planned sequence of HIP kernel launches (no autograd, no per-step allocation).

The plan is built once for a (model, batch size) pair:
  * every activation / gradient buffer is preallocated NHWC in HBM and reused across steps;
  * every parameter gradient is written exactly once, directly into the optimiser's flat gradient
    arena (no zero_grad pass, no accumulate pass) -- the arena is then all-reduced once (RCCL) and
    consumed by the fused optimiser kernel;
  * the launch list is replayable and hipGraph-capturable (``capture()``); the eager form stays the default because it runs
    the weight gradients on a side stream underneath the main chain, which a replayed graph serialises;
  * three arithmetic modes (``precision=``): exact fp32, split-bf16 (three MFMAs per product) and fp16 pairs with two MFMAs per
    product on the backward layers.

It drives the same C-ABI entry points as the autograd modules and must produce identical
gradients (tests/test_gpu_engine.py).  Reference path replaced: the loop body train_BE.py:54-64
with the model/loss of models/networks.py (Encoder :72-78, reparameterize :228-231, Decoder
:107-112, KL :270) and F.binary_cross_entropy.
"""
from __future__ import annotations

import math
import os
from ctypes import c_void_p
from typing import Dict, Optional

import torch

from . import _lib, ops, parallel, sections
from .networks import VAE
from .plan import PlanBuilder, _Plan, _ptr, plan_device, side_ctx, sync_counters_on_state_dict


class FusedVAEStep:
    """forward + loss + backward (+ all-reduce + optimiser) for a ``networks.VAE``.

    ``optimizer`` must be a flat-arena optimiser from ``vae_play_amd.optim`` built over
    ``vae.parameters()`` (its gradient arena receives the gradients).
    """

    def __init__(self, vae: VAE, optimizer, batch_size: int, img_size: int, channels: int, group=None,
                 precision: str = "bf16x3", grad_scale16: float = 4096.0, _plan_only: bool = False):
        """precision: "f32"    -- every contraction on v_mfma_f32_32x32x2_f32 (exact fp32, ~1e-6 parity);
                      "bf16x3" -- 5x5 convolutions whose channel counts are multiples of 8 run on the
                                  split-bf16 kernel (3 bf16 MFMAs per product, fp32 accumulate, ~1e-5 parity);
                                  edge layers and dense layers stay on the f32 kernels;
                      "f16x2"  -- the same plan with those convolutions on fp16-pair operands: forward layers with 3 fp16 MFMAs
                                  per product (outputs keep the ~1e-5 parity), BACKWARD layers (input and weight gradients) with
                                  2 (DECLARED tolerance ~2e-4 relative per layer on gradients; the final convolution's narrow
                                  side stays on its bf16x3 kernels).  ``grad_scale16`` (a power of two) is the factor
                                  gradient operands are multiplied by before they are written as fp16 pairs -- the consuming
                                  launch divides it out of its accumulators, so every fp32 buffer and the gradient arena hold
                                  true values; gradient elements beyond 65504 / grad_scale16 saturate."""
        if precision not in ("f32", "bf16x3", "f16x2"):
            raise ValueError("precision must be 'f32', 'bf16x3' or 'f16x2'")
        if precision == "f16x2" and not (grad_scale16 > 0 and math.log2(grad_scale16).is_integer()):
            raise ValueError("grad_scale16 must be a positive power of two")
        self.precision = precision
        self.grad_scale16 = float(grad_scale16)
        self.vae, self.opt, self.B, self.S, self.C = vae, optimizer, batch_size, img_size, channels
        self.Z, self.L = vae.z_size, vae.iter_level
        self.group = group
        self.world = torch.distributed.get_world_size(group) if torch.distributed.is_initialized() else 1
        self.opt.grad_scale = 1.0 / self.world
        self.dev = plan_device(vae, "FusedVAEStep", _plan_only)     # (_plan_only: the launch list over host buffers, for tests)
        self._bufs: Dict[str, torch.Tensor] = {}
        self._graph = None
        self.reload_switches()
        self._build()
        self._sd_hook = sync_counters_on_state_dict(self, vae)

    def reload_switches(self) -> None:
        """The A/B switches that shape a STEP (as opposed to the plan, which reads its own in ``_build``) are resolved here, once,
        when the engine is built -- not on every ``step()``.  The in-process A/B tools (tools/ab_env.py) call this again after
        flipping an environment variable."""
        env = os.environ.get
        self._side_wgrad = env("VP_SIDE_WGRAD", "1") != "0"          # weight gradients on the side stream
        self._adam_outer = env("VP_ADAM_OUTER", "1") != "0"          # one rank: fc.0's update contracted from its factors
        self._adam_outer_early = int(env("VP_ADAM_OUTER_EARLY", "2"))  # 0 end of step | 1 fc.0 early | 2 fc.0 + the slice behind it
        self._dp_factored = env("VP_DP_FACTORED", "1") != "0"        # several ranks: fc.0's gradient exchanged as its factors
        self._dp_enc_tail = env("VP_DP_ENC_TAIL", "1") != "0"        # several ranks: the deep encoder convs in their own bucket

    # ---- plan construction ------------------------------------------------------------------
    def _build(self):
        B, S, C, Z, L = self.B, self.S, self.C, self.Z, self.L
        enc, dec = self.vae.encoder, self.vae.decoder
        env = os.environ.get
        fwd, bwd = _Plan(), _Plan()
        P = _ptr
        # sticky device flag: the BatchNorm backward clamped a value of its fp16 gradient planes (|g| * grad_scale16 > 65504); read in
        # sync_counters()
        self._f16_sat = torch.zeros(1, dtype=torch.int32, device=self.dev)
        x3 = self.precision in ("bf16x3", "f16x2")
        # Weight gradients go to a side stream (bf16x3 plans): they only feed the optimiser, so they can run underneath
        # the next layer's HBM-bound BatchNorm backward.
        # (exact-f32 plans keep everything on the main stream: with their weight gradients on the side stream -- fp32 output gradients
        # rotating over two buffers, 128 / 160 / 192 CUs -- the step measured 8.39 / 8.06 / 8.03 ms against 7.89 ms in line; with only
        # the bandwidth-bound glue there -- slab reductions, final conv's VALU weight gradient, weight re-pack, early Adam slices, one
        # category at a time -- 7.72 - 7.79 ms against 7.66 in line: beside an fp32-MFMA kernel ANY second kernel costs more than it
        # hides, profiles/r03_notes.md sections 2 and 8)
        # CU budget of a weight gradient: the whole chip on the main stream, WGRAD_SIDE_CUS beside the main stream's kernels
        # (VP_WGRAD_MAIN_CUS, tests: the same budget on both streams = the same arithmetic)
        b = PlanBuilder(self, self.dev, self.precision, side_on=x3,
                        wgrad_cus=(int(env("VP_WGRAD_MAIN_CUS", "0")), int(env("VP_WGRAD_SIDE_CUS", "160"))),
                        grad_scale16=self.grad_scale16, sat=self._f16_sat, fuse_stats=env("VP_FUSE_BN_STATS", "1") != "0")
        lib = b.lib

        # ---------------- forward: stem / encoder blocks -> head -> trunk -> loss ----------------
        self.x_nchw = b.buf("x_nchw", B, C, S, S)
        self.eps = b.buf("eps", B, Z)
        x_nhwc = b.buf("x_nhwc", B * S * S * C)
        if C > 1:
            fwd.add("vp_nchw_to_nhwc_f32", P(self.x_nchw), P(x_nhwc), B, C, S, S)
        else:
            x_nhwc = self.x_nchw  # identical memory order for one channel
        blocks = sections.gather_stack(b, "enc", enc.conv, B, S, x_nhwc, None, image=self.x_nchw)
        for i, blk in enumerate(blocks):
            if i == 1 and b.k_pack is not None:
                fwd.wait_side(b.k_pack)
            blk.fwd(fwd)
        if L == 1 and b.k_pack is not None:
            fwd.wait_side(b.k_pack)
        head = sections.EncoderHead(b, enc, B, blocks[-1].Cout)
        head.fwd(fwd, blocks[-1].a)
        head.latent(fwd, self.eps)
        self.mu, self.logvar, self.z, self.kl = head.mu, head.logvar, head.z, head.kl
        # (spare_p1, and shared_colsum_ws below: kept so that this plan's buffers and launches stay as they are)
        trunk = sections.DecoderTrunk(b, dec, B, L, S, C, spare_p1=True)
        fin, Cf = trunk.fin, trunk.ch[-1]
        xt_nhwc = b.buf("xt_nhwc", B * S * S * C)
        dec_pass = trunk.fwd(fwd, "dec", self.z, xt_nhwc, "fin")
        self.recon = b.buf("recon", 1)
        self.kl_sum = b.buf("kl_sum", 1)
        n_pix = B * S * S * C
        ws_red = b.ws("red.ws", lib.vp_reduce_workspace_bytes(n_pix))
        self._loss_num = b.buf("loss_num", 1)
        fwd.add("vp_vae_loss_f32", P(xt_nhwc), P(x_nhwc), n_pix, P(self.kl), B, P(self.recon), P(self.kl_sum), P(self._loss_num),
                1.0 / B, P(ws_red), ws_red.numel() * 4)
        self.xt_nhwc = xt_nhwc
        self.x_tilde = xt_nhwc.view(B, S, S, C).permute(0, 3, 1, 2)  # logical NCHW, channels_last memory
        fwd.hook("fwd_done")

        # ---------------- backward: the reverse walk ----------------
        inv_b = 1.0 / B
        dlogit = b.buf("g.dlogit", n_pix)
        if fin.dlogit_s is not None:      # the final conv's input gradient reads dlogit padded to 8 channels, as split planes
            bwd.add("vp_bce_sigmoid_bwd_pad_split_f32", P(xt_nhwc), P(x_nhwc), inv_b, P(dlogit), P(fin.dlogit_s), B * S * S, C, 8)
        else:
            bwd.add("vp_bce_sigmoid_bwd_f32", P(xt_nhwc), P(x_nhwc), inv_b, P(dlogit), n_pix)
        b.wgrad_workspace([(B, k.Hs, k.Cin, k.Cout) for k in blocks] + [(B, Hs, Cout, Cin) for Hs, Cin, Cout in trunk.layers],
                          at_least=lib.vp_conv5_wgrad_workspace_bytes(B, S, S, Cf, C, 1))
        # two ping-pong gradient buffers sized for the largest activation
        big = max([B * head.F0, B * trunk.F1, n_pix, B * S * S * Cf] + [B * 4 * Hs * Hs * Cout for Hs, _, Cout in trunk.layers]
                  + [k.R * k.Cout for k in blocks])
        gA, gB = b.buf("g.A", big), b.buf("g.B", big)
        planes = b.grad_planes(big)       # split gradient (output of BN backward) for the 16-bit kernels
        self._grad_planes = planes if b.x2 else []
        dz = b.buf("g.dz", B, Z)
        trunk.bwd(bwd, dec_pass, dlogit, gA, gB, dz=dz)
        # every decoder gradient is final and no decoder parameter is read any more: the data-parallel step may start
        # reducing that slice of the arena and the optimiser may update it
        bwd.hook("dec_done")
        head.bwd(bwd, self.eps, dz, inv_b, gA, gB, fc_wgrad_hook=True, shared_colsum_ws=True)
        self._fc_factors = (head.dh, head.flat, head.fc_lin.weight, head.F0)
        # the encoder-tail bucket: its hook's index in the backward plan and the first of the blocks it covers (None: no such bucket)
        self._bwd_b_enc_tail = self._enc_tail_first = None
        for i in range(L - 1, -1, -1):
            blocks[i].bwd(bwd, gB, gA)
            if blocks[i].is16 and i == max(L - 2, 1):
                # the gradients of encoder.conv[i:] (16.4 of the 17 MB of conv parameters at config 3) are issued: third bucket
                self._bwd_b_enc_tail, self._enc_tail_first = len(bwd.calls), i
                bwd.hook("enc_tail")
        b.finish(fwd)
        self._fwd, self._bwd = fwd, bwd
        self._bn_momentum_eps = {id(bn): (float(bn.momentum), float(bn.eps)) for bn, _ in b.bn_counts}
        self._bn_mods = [m for m in self.vae.modules() if hasattr(m, "num_batches_tracked")]

    # ---- execution ---------------------------------------------------------------------------
    def _launch_all(self, timers: Optional[dict] = None, hooks: Optional[dict] = None):
        s = torch.cuda.current_stream().cuda_stream
        # instrumented steps run the serial schedule: an event pair around a kernel that shares the GPU with another
        # stream's kernels would time the mixture, not the kernel
        side = self._side_ctx() if timers is None else None
        self._fwd.run(s, timers, side=side, hooks=hooks)
        self._bwd.run(s, timers, side=side, hooks=hooks)
        if side is not None:
            side.join()

    def _side_ctx(self):
        """the side stream when weight gradients run concurrently (bf16x3 / f16x2 plans, VP_SIDE_WGRAD != 0), else None"""
        return side_ctx(self, self._side_wgrad)

    def forward_backward(self, x: torch.Tensor, eps: torch.Tensor, timers: Optional[dict] = None, hooks: Optional[dict] = None):
        """Gradients of (BCE_sum + KL_sum)/B land in the optimiser's flat gradient arena.
        Returns (loss, recon, kl) as device scalars (no host sync).  They are the plan's static output buffers (like the
        outputs of a captured graph): the next step overwrites them, so read or copy them before stepping again.  ``timers`` =
        {"names": set of entry points, "events": []} brackets those launches with HIP events
        (eager mode only).  ``hooks`` = {name: fn(side)}: called at the plan's named points with the side stream (or None) --
        "fwd_done" after the forward; "dec_done" once every decoder gradient is launched; "fc_wgrad" INSTEAD of encoder.fc.0's
        weight-gradient GEMM; "enc_dense_done" after the encoder's dense layers; "enc_tail" once the deep encoder blocks'
        gradients are launched (split-operand plans only, ``_bwd_b_enc_tail`` = that hook's index in ``_bwd``)."""
        self._bind_inputs(x, eps)
        if self._graph is not None and timers is None and not hooks:
            self._graph.replay()
        else:
            self._launch_all(timers, hooks)
        # the plan wrote every gradient into the arena: a ``.grad`` left None by zero_grad(set_to_none=True) must not read as
        # "no gradient" in the optimiser's gather_grads()
        self.opt.arena.adopt_views()
        # BatchNorm num_batches_tracked is advanced lazily in sync_counters()
        self._steps_since_sync = getattr(self, "_steps_since_sync", 0) + 1
        return self._loss_num, self.recon, self.kl_sum     # (loss per image, recon sum, KL sum): device scalars of the plan

    def _bind_inputs(self, x: torch.Tensor, eps: torch.Tensor) -> None:
        """Point the launches that consume the batch at the caller's tensors (fp32, contiguous, on this device, right shape:
        the three-channel transpose reads ``x``, the two latent kernels read ``eps``); anything else -- and the hipGraph
        replay, whose node arguments are frozen -- is copied into the plan's static buffers."""
        if not hasattr(self, "_in_slots"):
            self._in_slots = {"x": [], "eps": []}
            statics = {"x": self.x_nchw.data_ptr(), "eps": self.eps.data_ptr()}
            if self.C != 1:                  # one channel: x_nchw doubles as the NHWC activation of the whole plan
                for plan in (self._fwd, self._bwd):
                    for call in plan.calls:
                        for i, a in enumerate(call[2]):
                            if isinstance(a, c_void_p):
                                for k, v in statics.items():
                                    if a.value == v:
                                        self._in_slots[k].append((call[2], i))
        for key, t, static in (("x", x, self.x_nchw), ("eps", eps, self.eps)):
            if tuple(t.shape) != tuple(static.shape):
                # (``static.copy_(t)`` would broadcast a (1, C, H, W) batch silently; a DataLoader's short last batch -- no
                # drop_last -- would raise a bare torch broadcast error)
                raise _lib.VaePlayHipError(
                    f"FusedVAEStep: {key} has shape {tuple(t.shape)}, this plan was built for {tuple(static.shape)} "
                    f"(batch {self.B}; build a second FusedVAEStep over the same optimiser for another batch size)")
            slots = self._in_slots[key]
            direct = (bool(slots) and self._graph is None and t.device == static.device and t.dtype == torch.float32
                      and t.is_contiguous() and t.shape == static.shape)
            if not direct:
                static.copy_(t, non_blocking=True)
                t = static
            for args, i in slots:
                args[i] = c_void_p(t.data_ptr())

    def f16_saturated(self) -> int:
        """precision="f16x2" diagnostics (a host sync; not on the step's path): how many elements of the fp16 gradient planes sit at
        +-65504, i.e. |g| * grad_scale16 overflowed fp16's range in the last step and was clamped.  The two ping-pong buffers hold
        the last two layers' planes (earlier layers were overwritten): a non-zero count means grad_scale16 is too large for this
        model / loss scale -- lower it (powers of two; 4096 leaves |g| < 16)."""
        n = 0
        for t in getattr(self, "_grad_planes", []):
            hi = t[0].view(torch.float16)
            n += int((hi.abs() >= 65504.0).sum().item())
        return n

    def sync_counters(self):
        """Advance BatchNorm ``num_batches_tracked`` buffers (bookkeeping only; kept off the hot path).  precision="f16x2": also reads
        the sticky saturation flag (a host sync, like everything here) and raises when a step since the last call clamped a gradient at
        +-65504 / grad_scale16 -- the weights of those steps are off; lower ``grad_scale16``.  The flag covers the fp16 gradient planes
        that the BatchNorm backward writes (csrc/bn.hip's tiled kernel, the only one with split planes); the planes of dlogit and of
        the NCHW -> NHWC pass do not report (``f16_saturated()`` counts clamped elements in whatever planes are still held)."""
        n = getattr(self, "_steps_since_sync", 0)
        if n:
            for m in self._bn_mods:
                m.num_batches_tracked.add_(n)
            self._steps_since_sync = 0
        if self.precision == "f16x2" and int(self._f16_sat.item()):
            self._f16_sat.zero_()
            raise _lib.VaePlayHipError(
                f"precision='f16x2': gradient planes saturated fp16's range since the last sync_counters() (|g| * grad_scale16 > 65504 "
                f"with grad_scale16 = {self.grad_scale16:g}); build the step with a smaller power of two")

    def _decoder_slice_start(self) -> int:
        """Arena offset of the first decoder parameter (encoder parameters precede it in ``vae.parameters()``)."""
        dec_ids = {id(p) for p in self.vae.decoder.parameters()}
        offs = [o for p, o in zip(self.opt.arena.params, self.opt.arena.offsets) if id(p) in dec_ids]
        first = min(offs)
        assert all(o >= first for o in offs) and all(
            (id(p) in dec_ids) == (o >= first) for p, o in zip(self.opt.arena.params, self.opt.arena.offsets)), \
            "decoder parameters must form the tail of the flat arena"
        return first

    def _encoder_dense_start(self) -> int:
        """Arena offset of ``encoder.fc.0.weight``: the encoder's conv/BN parameters precede it, its dense
        parameters (fc.0, fc.1, l_mu, l_var) run from there to the decoder slice."""
        a = self.opt.arena
        off = {id(p): o for p, o in zip(a.params, a.offsets)}
        first = off[id(self.vae.encoder.fc[0].weight)]
        conv_ids = {id(p) for p in self.vae.encoder.conv.parameters()}
        assert all((id(p) in conv_ids) == (o < first) for p, o in zip(a.params, a.offsets) if o < self._decoder_slice_start()), \
            "encoder conv parameters must form the head of the flat arena"
        return first

    def step(self, x: torch.Tensor, eps: torch.Tensor, timers: Optional[dict] = None, overlap: bool = True, comm_trace=None):
        """One full training step: fwd + loss + bwd, SUM all-reduce of the flat gradient arena, fused update.

        With several ranks the arena is reduced as four buckets of the same flat buffer, each handed to RCCL as
        soon as its gradients are final so that the all-reduce runs on the communicator's stream underneath the rest
        of backward: the decoder slice after the decoder's backward, the encoder's dense slice (fc.0 is 134 MB of the
        213 MB at config 3) after its weight gradient, the deep encoder blocks' conv slice (16.4 MB) while the shallow blocks
        still run backward, and the rest of the encoder's conv slice (< 1 MB) after backward; the
        optimiser kernel waits for all of them.  ``overlap=False`` issues one all-reduce of the whole arena.
        ``comm_trace`` (parallel.CommTrace, instrumented steps of bench.py): every collective is issued through it, which
        records its bytes, its device time and the time the main stream waits for collectives.
        (Updating each slice right after its all-reduce, on a second side stream underneath the rest of backward, was
        measured and is NOT done: the HBM-bound optimiser kernel slows the concurrent kernels by more than it hides,
        4.52 vs 4.46 ms/step on one GPU; ``optim.*.step_range`` remains available.)"""
        tr = comm_trace

        def reduce(name, t):         # SUM all-reduce of one bucket, issued now
            if tr is not None:
                return tr.issue(name, "all_reduce", t.numel() * 4, lambda: parallel.allreduce_flat_grads(t, self.group, async_op=True))
            return parallel.allreduce_flat_grads(t, self.group, async_op=True)

        def gather(name, out_all, local):
            if tr is not None:
                return tr.issue(name, "all_gather", out_all.numel() * 4,
                                lambda: parallel.allgather_rows(out_all, local, self.group, async_op=True))
            return parallel.allgather_rows(out_all, local, self.group, async_op=True)

        def wait_all(works):
            if tr is not None:
                tr.wait()
                return
            for w in works:
                if w is not None:
                    w.wait()

        if parallel.dp_active(self.group) and overlap:
            g = self.opt.flat_grad
            cut = self._decoder_slice_start()
            dense = self._encoder_dense_start()
            works = []
            factored = self._dp_factored

            def dec_bucket(side):
                if side is not None:                         # the decoder's weight gradients are produced on the side stream
                    side.join()
                works.append(reduce("decoder", g[cut:]))
            hooks = {"dec_done": dec_bucket}
            # fourth cut: encoder.conv[i:] for the deepest blocks -- almost all of the encoder's conv parameters -- is reduced
            # while the remaining shallow blocks still run backward, so that only their < 1 MB is left for the exposed
            # all-reduce at the end of the step.  Its weight gradients are produced on the side stream and its BatchNorm
            # gradients on the main stream: the collective is issued from the side stream after it has joined the main one.
            tail_lo = dense
            if self._enc_tail_first is not None and self._dp_enc_tail:
                off = {id(p): o for p, o in zip(self.opt.arena.params, self.opt.arena.offsets)}
                tail_lo = off[id(self.vae.encoder.conv[self._enc_tail_first].conv.weight)]
            if tail_lo < dense:
                def enc_tail(side):
                    def issue():
                        works.append(reduce("encoder.conv[deep]", g[tail_lo:dense]))
                    if side is not None:
                        side.run(issue)
                    else:
                        issue()
                hooks["enc_tail"] = enc_tail
            if factored:
                # fc.0's weight gradient (134 MB of the 213 MB at config 3) is dW = dh^T flat, a sum of B outer products
                # per rank: exchange the two factors (W x 4.3 MB all-gather) and contract over all W*B rows locally
                # instead of all-reducing the weight-sized result.  Identical to the sum of the ranks' gradients.
                dh, flat, fcw, F0 = self._fc_factors
                W, B = self.world, self.B
                if not hasattr(self, "_fc_all"):
                    self._fc_all = (torch.empty((W * B, 1024), device=self.dev), torch.empty((W * B, F0), device=self.dev))
                dh_all, flat_all = self._fc_all
                gathers = []
                fc_lo = self.opt.arena.offsets[[id(p) for p in self.opt.arena.params].index(id(fcw))]
                fc_hi = fc_lo + (fcw.numel() + 63) // 64 * 64

                def after_fwd(side):
                    gathers.append(gather("fc.0 factor: flat", flat_all, flat.view(B, F0)))

                def fc_wgrad(side):
                    gathers.append(gather("fc.0 factor: dh", dh_all, dh.view(B, 1024)))
                    wait_all(gathers)
                    ops.gemm(dh_all, 1, 1024, flat_all, 1, F0, 1024, F0, W * B, 2, out=self.opt.arena.grad_view(fcw).view(1024, F0))

                def dense_bucket(side):
                    assert fc_lo == dense, "fc.0.weight must open the encoder's dense slice"
                    works.append(reduce("encoder dense (without fc.0)", g[fc_hi:cut]))
                hooks.update(fwd_done=after_fwd, fc_wgrad=fc_wgrad, enc_dense_done=dense_bucket)
            else:
                hooks["enc_dense_done"] = lambda side: works.append(reduce("encoder dense", g[dense:cut]))
            out = self.forward_backward(x, eps, timers, hooks=hooks)
            works.append(reduce("encoder.conv[shallow]" if tail_lo < dense else "encoder.conv", g[:tail_lo]))
            wait_all(works)
        elif self.world == 1 and self._graph is None and self._outer_adam():      # (a captured graph replays the materialising plan)
            # one rank: encoder.fc.0's weight gradient (134 MB at config 3) is contracted from its two factors inside the Adam
            # kernel instead of being written by a GEMM and read back by the update; fc.0.weight.grad is NOT written by step()
            # (forward_backward() alone materialises every gradient).
            # ... and that update runs on the side stream as soon as its factors are final and the dense input gradient has read the
            # weight for the last time in this step: 134 us of HBM-bound work underneath the encoder's MFMA-bound convolution backward
            # instead of behind it (VP_ADAM_OUTER_EARLY=0: at the end of the step; 1: fc.0 only; 2, the default: fc.0 and the arena
            # slice behind it.  3.640 / 3.609 / 3.572 ms in one process, tools/ab_env.py)
            hooks = {"fc_wgrad": lambda side: None}
            if timers is None and self._adam_outer_early:
                def early(side):
                    if side is not None:
                        # (mode 2: also the arena slice behind fc.0 -- the rest of the encoder's dense layers and the whole decoder,
                        # whose weight gradients precede this launch on the side stream and whose other gradients the fork covers)
                        side.run(lambda: self.opt.step_outer_early(
                            with_tail=(self._adam_outer_early == 2 and getattr(self, "_early_tail_ok", False))))
                hooks["enc_dense_done"] = early
            out = self.forward_backward(x, eps, timers, hooks=hooks)
            self.opt.step(outer=True)
            return out
        else:
            out = self.forward_backward(x, eps, timers)
            if parallel.dp_active(self.group):
                wait_all([reduce("whole gradient arena", self.opt.flat_grad)])
        if tr is not None:
            tr.end_step()
        self.opt.step()
        return out

    def _outer_adam(self) -> bool:
        if not self._adam_outer or not hasattr(self.opt, "set_outer_grad"):
            return False
        # the factors are THIS engine's static buffers: bind them on every call in which the optimiser holds another engine's
        # (a second FusedVAEStep over the same optimiser -- another batch size, precision or a rebuilt plan -- would otherwise
        # have its fc.0 update contracted from the first engine's stale buffers)
        dh, flat, fcw, F0 = self._fc_factors
        cur = getattr(self.opt, "_outer", None)
        if cur is None or cur[4].data_ptr() != dh.data_ptr() or cur[5].data_ptr() != flat.data_ptr() or cur[4].shape[0] != self.B:
            self.opt.set_outer_grad(fcw, dh.view(self.B, 1024), flat.view(self.B, F0))
        if not hasattr(self, "_early_tail_ok"):
            # the early update of the arena slice BEHIND fc.0 (step()) relies on the arena order of vae.parameters(): encoder conv
            # blocks, fc.0, the encoder's other dense layers, the decoder
            try:
                self._early_tail_ok = self._encoder_dense_start() == self.opt._outer[0]
            except AssertionError:
                self._early_tail_ok = False
        return True

    def capture(self, warmup: int = 2):
        """Capture forward+backward into a hipGraph (torch.cuda.CUDAGraph) and replay it from then on."""
        self._bind_inputs(self.x_nchw, self.eps)      # the graph's nodes must read the static buffers
        # warm-up and capture execute the step: keep the BatchNorm running buffers unchanged by them
        saved = [(m, m.running_mean.clone(), m.running_var.clone()) for m in self._bn_mods]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._launch_all()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        ops.CAPTURE_OK[0] = True          # (ops._stream() refuses captures it does not know: the autograd front end's)
        try:
            with torch.cuda.graph(g):
                self._launch_all()
        finally:
            ops.CAPTURE_OK[0] = False
        self._graph = g
        for m, rm, rv in saved:
            m.running_mean.copy_(rm)
            m.running_var.copy_(rv)
        return g
