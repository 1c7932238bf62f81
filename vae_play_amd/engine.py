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

from . import _lib, ops, parallel
from .networks import VAE
from .plan import FWD_PRODUCTS, PlanBuilder, _Plan, _ptr, grad_of, plan_device, side_ctx, sync_counters_on_state_dict

_ACT_NONE, _ACT_SIGMOID = ops.ACT_NONE, ops.ACT_SIGMOID


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
        # sticky device flag: a producer of fp16 gradient planes clamped a value (|g| * grad_scale16 > 65504); read in sync_counters()
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
        x2 = b.x2                                      # fp16-pair planes + the *_f16x2 launches (same plan structure)
        FMT = 1 if x2 else 0                           # VP_SPLIT_F16 | VP_SPLIT_BF16
        GS = b.GS
        a16 = self.precision if x3 else "f32"          # arithmetic of the 5x5 layers whose channel counts are multiples of 8

        def use16(cin, cout):
            return x3 and cin % 8 == 0 and cout % 8 == 0

        # ---------------- forward ----------------
        self.x_nchw = b.buf("x_nchw", B, C, S, S)
        self.eps = b.buf("eps", B, Z)
        x_nhwc = b.buf("x_nhwc", B * S * S * C)
        if C > 1:
            fwd.add("vp_nchw_to_nhwc_f32", P(self.x_nchw), P(x_nhwc), B, C, S, S)
        else:
            x_nhwc = self.x_nchw  # identical memory order for one channel

        enc_ch = [C] + [blk.conv.weight.shape[0] for blk in enc.conv]
        sp = [S // (2 ** i) for i in range(L + 1)]
        enc16 = [use16(enc_ch[i], enc_ch[i + 1]) for i in range(L)]
        enc0_cols = x3 and C in (1, 3) and enc_ch[1] % 8 == 0
        # exact f32: the same im2col as plain fp32, both 1x1 layers on the fp32-MFMA kernels (the 3-channel implicit GEMM and the VALU
        # weight gradient took 48 + 67 us at the benchmark shard, the two 1x1 layers 36 + 40 + 20 us of im2col / re-order: 7.63 -> 7.60 ms)
        enc0_cols32 = (not x3) and C in (1, 3) and enc_ch[1] % 16 == 0
        enc_in = [x_nhwc]        # fp32 inputs (None when only the split copy exists)
        enc_in_s = [None]        # split inputs
        enc_rec = []
        for i, blk in enumerate(enc.conv):
            if i == 1 and b.k_pack is not None:
                fwd.wait_side(b.k_pack)
            Cin, Cout, Hs = enc_ch[i], enc_ch[i + 1], sp[i + 1]
            n_out = B * Hs * Hs * Cout
            c = b.buf(f"enc{i}.c", n_out)
            fl = 50.0 * B * Hs * Hs * Cin * Cout
            geom = (B, Hs, Hs, Cin, Cout, 2)
            conv = None
            if i == 0 and enc0_cols:
                # first conv (1 or 3 image channels): im2col written once as split planes, then a 1x1 layer on the MFMA kernels
                KC = lib.vp_im2col5s2_cols(Cin)
                xcol = b.sbuf("enc0.xcol", B * Hs * Hs * KC)
                w0s = b.sbuf("enc0.w0s", Cout * KC)
                if x2:
                    fwd.add("vp_im2col5s2_split_fmt_f32", P(self.x_nchw), P(xcol), B, Cin, S, S, 1, FMT)
                    fwd.add("vp_pack_w_im2col5_split_fmt", P(blk.conv.weight), P(w0s), Cout, Cin, FMT)
                    fwd.add("vp_conv_gather_f16", P(xcol), P(w0s), None, P(c), B, Hs, Hs, Hs, Hs, KC, Cout, 1, 1, _ACT_NONE, FWD_PRODUCTS, 1.0,
                            flops=fl, tag="enc0.fwd")
                else:
                    fwd.add("vp_im2col5s2_split_f32", P(self.x_nchw), P(xcol), B, Cin, S, S, 1)
                    fwd.add("vp_pack_w_im2col5_split", P(blk.conv.weight), P(w0s), Cout, Cin)
                    fwd.add("vp_conv_gather_bf16x3", P(xcol), P(w0s), None, P(c), B, Hs, Hs, Hs, Hs, KC, Cout, 1, 1, _ACT_NONE,
                            flops=fl, tag="enc0.fwd")
                p1, enc0 = None, (xcol, KC)
            elif i == 0 and enc0_cols32:
                KC = lib.vp_im2col5s2_cols(Cin)
                xcol = b.buf("enc0.xcol32", B * Hs * Hs * KC)
                w0 = b.buf("enc0.w0", Cout * KC)
                fwd.add("vp_im2col5s2_f32", P(self.x_nchw), P(xcol), B, Cin, S, S, 1)
                fwd.add("vp_pack_w_im2col5_f32", P(blk.conv.weight), P(w0), Cout, Cin)
                fwd.add("vp_conv_gather_f32", P(xcol), P(w0), None, P(c), B, Hs, Hs, Hs, Hs, KC, Cout, 1, 1, _ACT_NONE, flops=fl, tag="enc0.fwd")
                p1, enc0 = None, (xcol, KC)
            elif enc16[i]:
                p0 = b.sbuf(f"enc{i}.p0s", Cout * 25 * Cin)
                p1 = b.sbuf(f"enc{i}.p1s", Cin * 25 * Cout)
                b.pack(blk.conv.weight, p0, p1, Cout, Cin, True, first=(i == 0))
                conv = (0, a16, enc_in_s[-1], p0, geom, fl)
            else:
                p0 = b.buf(f"enc{i}.p0", Cout * 25 * Cin)
                p1 = b.buf(f"enc{i}.p1", Cin * 25 * Cout) if i > 0 else None
                b.pack(blk.conv.weight, p0, p1, Cout, Cin, False, first=(i == 0))
                conv = (0, "f32", enc_in[-1], p0, geom, fl)
            # the activation feeds the next conv (+ its wgrad) or, for the last block, the flatten
            nxt16 = i + 1 < L and enc16[i + 1]
            a = None if nxt16 else b.buf(f"enc{i}.a", n_out)
            a_s = b.sbuf(f"enc{i}.as", n_out) if nxt16 else None
            saved = b.bn_fwd(fwd, f"enc{i}", c, B * Hs * Hs, Cout, blk.bn, a, a_s, conv=conv)
            enc_rec.append((blk, Cin, Cout, Hs, p1, c, saved))
            enc_in.append(a)
            enc_in_s.append(a_s)
        if L == 1 and b.k_pack is not None:
            fwd.wait_side(b.k_pack)
        size = enc_ch[-1]
        F0 = 64 * size
        flat = b.buf("enc.flat", B * F0)
        fwd.add("vp_nhwc_to_nchw_f32", P(enc_in[-1]), P(flat), B, size, 8, 8)
        fc_lin, fc_bn = enc.fc[0], enc.fc[1]
        h = b.buf("enc.h", B * 1024)
        hb = b.buf("enc.hb", B * 1024)
        b.lin_fwd(fwd, flat, fc_lin.weight, None, h, B, 1024, F0)
        h_saved = b.bn_fwd(fwd, "enc.fc", h, B, 1024, fc_bn, hb)
        self.mu, self.logvar = b.buf("mu", B, Z), b.buf("logvar", B, Z)
        for lin, out in ((enc.l_mu, self.mu), (enc.l_var, self.logvar)):
            b.lin_fwd(fwd, hb, lin.weight, lin.bias, out, B, Z, 1024)
        self.z, self.kl = b.buf("z", B, Z), b.buf("kl", B)
        fwd.add("vp_latent_fwd_f32", P(self.mu), P(self.logvar), P(self.eps), P(self.z), P(self.kl), B, Z)

        dfc_lin, dfc_bn = dec.fc[0], dec.fc[1]
        dsize = dec._c0
        F1 = 64 * dsize
        d = b.buf("dec.d", B * F1)
        db = b.buf("dec.db", B * F1)
        b.lin_fwd(fwd, self.z, dfc_lin.weight, None, d, B, F1, Z)
        d_saved = b.bn_fwd(fwd, "dec.fc", d, B, F1, dfc_bn, db)
        dec_ch = [dsize] + [blk.conv.weight.shape[1] for blk in list(dec.conv)[:L]]
        dec16 = [use16(dec_ch[i], dec_ch[i + 1]) for i in range(L)]
        dn = None if dec16[0] else b.buf("dec.in", B * F1)
        dn_s = b.sbuf("dec.in_s", B * F1) if dec16[0] else None
        if x2:
            fwd.add("vp_nchw_to_nhwc_split_fmt_f32", P(db), P(dn), P(dn_s), B, dsize, 8, 8, FMT)
        else:
            fwd.add("vp_nchw_to_nhwc_split_f32", P(db), P(dn), P(dn_s), B, dsize, 8, 8)

        dec_in = [dn]
        dec_in_s = [dn_s]
        dec_rec = []
        for i in range(L):
            blk = dec.conv[i]
            Cin, Cout, Hs = dec_ch[i], dec_ch[i + 1], 8 * (2 ** i)
            n_out = B * 4 * Hs * Hs * Cout
            tbuf = b.buf(f"dec{i}.t", n_out)
            fl = 50.0 * B * Hs * Hs * Cin * Cout
            geom = (B, Hs, Hs, Cin, Cout, 2)
            if dec16[i]:
                p1 = b.sbuf(f"dec{i}.p1s", Cout * 25 * Cin)   # T family: [Cbig=Cout][25][Csmall=Cin]
                p0 = b.sbuf(f"dec{i}.p0s", Cin * 25 * Cout)   # F family (dgrad): [Csmall=Cin][25][Cbig=Cout]
                b.pack(blk.conv.weight, p0, p1, Cin, Cout, True)
                conv = (1, a16, dec_in_s[-1], p1, geom, fl)
            else:
                p1 = b.buf(f"dec{i}.p1", Cout * 25 * Cin)
                p0 = b.buf(f"dec{i}.p0", Cin * 25 * Cout)
                b.pack(blk.conv.weight, p0, p1, Cin, Cout, False)
                conv = (1, "f32", dec_in[-1], p1, geom, fl)
            # the last block feeds the final conv in fp32 (its 3-channel side runs on the VALU kernels of narrow.hip;
            # measured: padding 3 -> 32 output columns for the MFMA halo kernel is LDS-read bound and 25 % slower)
            nxt16 = i + 1 < L and dec16[i + 1]
            u = None if nxt16 else b.buf(f"dec{i}.u", n_out)
            u_s = b.sbuf(f"dec{i}.us", n_out) if nxt16 else None
            saved = b.bn_fwd(fwd, f"dec{i}", tbuf, B * 4 * Hs * Hs, Cout, blk.bn, u, u_s, conv=conv)
            dec_rec.append((blk, Cin, Cout, Hs, p0, tbuf, saved))
            dec_in.append(u)
            dec_in_s.append(u_s)
        fin = dec.conv[L][0]
        Cf = dec_ch[-1]
        fl_fin = 50.0 * B * S * S * Cf * C
        fp0 = b.buf("fin.p0", C * 25 * Cf)
        fp1 = b.buf("fin.p1", Cf * 25 * C)
        b.pack(fin.weight, fp0, fp1, C, Cf, False)
        xt_nhwc = b.buf("xt_nhwc", B * S * S * C)
        if x3 and Cf == 64 and C in (1, 3):
            # split-bf16 on the matrix cores, taps folded into the MFMA columns (the exact-f32 plan keeps the VALU kernel)
            fwd.add("vp_conv5_smallout_bf16x3", P(dec_in[-1]), P(fp0), P(fin.bias), P(xt_nhwc), B, S, S, Cf, C, _ACT_SIGMOID,
                    flops=fl_fin, tag="fin.fwd")
        else:
            b.conv5(fwd, 0, "f32", dec_in[-1], fp0, xt_nhwc, (B, S, S, Cf, C, 1), bias=fin.bias, act=_ACT_SIGMOID,
                    flops=fl_fin, tag="fin.fwd")
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

        # ---------------- backward ----------------
        inv_b = 1.0 / B
        dlogit = b.buf("g.dlogit", n_pix)
        # final conv's input gradient: rows-in-K kernel of edge.hip (C = 1 | 3 image channels, 64 decoder channels), else the bf16x3
        # halo kernel with dlogit padded to 8 channels
        fin_rowk = x3 and Cf == 64 and C in (1, 3)
        fin16 = x3 and Cf % 8 == 0 and C < 8 and not fin_rowk
        if fin16:
            dlogit_s = b.sbuf("g.dlogit_s", B * S * S * 8)
            fp1s = b.sbuf("fin.p1s", Cf * 25 * 8)
            b.pack(fin.weight, None, fp1s, C, Cf, True, 8, bf16=True)       # bf16 pairs: read by the halo kernel in every mode
            bwd.add("vp_bce_sigmoid_bwd_pad_split_f32", P(xt_nhwc), P(x_nhwc), inv_b, P(dlogit), P(dlogit_s), B * S * S, C, 8)
        else:
            bwd.add("vp_bce_sigmoid_bwd_f32", P(xt_nhwc), P(x_nhwc), inv_b, P(dlogit), n_pix)
        b.colsum(bwd, "g.fin", dlogit, grad_of(fin.bias), B * S * S, C, side=b.side_slot())
        ws_wg = b.wgrad_workspace([(B, r[3], r[1], r[2]) for r in enc_rec] + [(B, r[3], r[2], r[1]) for r in dec_rec],
                                  at_least=lib.vp_conv5_wgrad_workspace_bytes(B, S, S, Cf, C, 1))
        n_tapm = lib.vp_conv5_smallout_wgrad_bf16x3_workspace_bytes(B, S, S, Cf, C)      # (the exact-f32 form takes the same slabs)
        if n_tapm:      # on the matrix cores, taps folded into the MFMA rows (csrc/edge.hip); its own slab workspace
            ws_fw = b.ws("g.finwgrad.ws", n_tapm)
            bwd.add("vp_conv5_smallout_wgrad_bf16x3" if x3 else "vp_conv5_smallout_wgrad_f32", P(dec_in[-1]), P(dlogit), P(grad_of(fin.weight)),
                    B, S, S, Cf, C, P(ws_fw), ws_fw.numel() * 4, flops=fl_fin, tag="fin.wgrad", side=b.side_slot())
        else:
            bwd.add("vp_conv5_wgrad_f32", P(dec_in[-1]), P(dlogit), P(grad_of(fin.weight)), B, S, S, Cf, C, 1, P(ws_wg), ws_wg.numel() * 4,
                    flops=fl_fin, tag="fin.wgrad", side=b.side_slot())   # reads dlogit / dec_in[-1]: both live on
        # two ping-pong gradient buffers sized for the largest activation
        big = max([B * F0, B * F1, n_pix] + [B * 4 * r[3] * r[3] * r[2] for r in dec_rec] + [B * r[3] * r[3] * r[2] for r in enc_rec]
                  + [B * S * S * Cf])
        gA, gB = b.buf("g.A", big), b.buf("g.B", big)
        if fin_rowk:
            bwd.add("vp_conv5_smallin_dgrad_bf16x3", P(dlogit), P(fin.weight), P(gA), B, S, S, C, Cf, flops=fl_fin, tag="fin.dgrad")
        elif fin16:
            b.conv5(bwd, 1, "bf16x3", dlogit_s, fp1s, gA, (B, S, S, 8, Cf, 1), flops=fl_fin, tag="fin.dgrad")
        elif Cf == 64 and C in (1, 3):    # exact fp32 on the same rows-in-K tiling (csrc/edge.hip dgrad_rowk_f32_kernel)
            bwd.add("vp_conv5_smallin_dgrad_f32", P(dlogit), P(fin.weight), P(gA), B, S, S, C, Cf, flops=fl_fin, tag="fin.dgrad")
        else:
            b.conv5(bwd, 1, "f32", dlogit, fp1, gA, (B, S, S, C, Cf, 1), flops=fl_fin, tag="fin.dgrad")
        cur, other = gA, gB
        gS2 = b.grad_planes(big)          # split gradient (output of BN backward) for the 16-bit kernels
        self._grad_planes = gS2 if x2 else []
        for i in range(L - 1, -1, -1):
            blk, Cin, Cout, Hs, p0, tbuf, saved = dec_rec[i]
            R = B * 4 * Hs * Hs
            fl = 50.0 * B * Hs * Hs * Cin * Cout
            geom = (B, Hs, Hs, Cout, Cin, 2)
            if dec16[i]:
                k, gS = b.next_plane(bwd)
                b.bn_bwd(bwd, tbuf, cur, None, R, Cout, blk.bn, saved, gS)                      # gS = d t_i (split)
                b.wgrad5(bwd, gS, dec_in_s[i], grad_of(blk.conv.weight), geom, k, flops=fl, tag=f"dec{i}.wgrad")
                b.conv5(bwd, 0, a16, gS, p0, cur, geom, products=2, alpha=1.0 / GS, flops=fl, tag=f"dec{i}.dgrad")  # cur = d input_i
            else:
                b.bn_bwd(bwd, tbuf, cur, other, R, Cout, blk.bn, saved)                         # other = d t_i
                bwd.add("vp_conv5_wgrad_f32", P(other), P(dec_in[i]), P(grad_of(blk.conv.weight)), *geom,
                        P(ws_wg), ws_wg.numel() * 4, flops=fl, tag=f"dec{i}.wgrad")
                b.conv5(bwd, 0, "f32", other, p0, cur, geom, flops=fl, tag=f"dec{i}.dgrad")     # cur = d input_i
        bwd.add("vp_nhwc_to_nchw_f32", P(cur), P(other), B, dsize, 8, 8)                # other = d db  (B, F1)
        b.bn_bwd(bwd, d, other, cur, B, F1, dfc_bn, d_saved)                           # cur = d d
        b.lin_wgrad(bwd, cur, self.z, grad_of(dfc_lin.weight), B, F1, Z)
        dz = b.buf("g.dz", B, Z)
        b.lin_dgrad(bwd, cur, dfc_lin.weight, dz, B, F1, Z)
        # every decoder gradient is final and no decoder parameter is read any more: the data-parallel step may start
        # reducing that slice of the arena and the optimiser may update it
        bwd.hook("dec_done")
        dmu, dlv = b.buf("g.dmu", B, Z), b.buf("g.dlv", B, Z)
        bwd.add("vp_latent_bwd_f32", P(self.mu), P(self.logvar), P(self.eps), P(dz), None, inv_b, P(dmu), P(dlv), B, Z)
        dhb_a, dhb_b = b.buf("g.dhb_a", B * 1024), b.buf("g.dhb_b", B * 1024)
        for lin, dsrc, dst in ((enc.l_mu, dmu, dhb_a), (enc.l_var, dlv, dhb_b)):
            b.lin_wgrad(bwd, dsrc, hb, grad_of(lin.weight), B, Z, 1024)
            b.colsum(bwd, "g.heads", dsrc, grad_of(lin.bias), B, Z)
            b.lin_dgrad(bwd, dsrc, lin.weight, dst, B, Z, 1024)
        bwd.add("vp_add_f32", P(dhb_a), P(dhb_b), P(dhb_a), B * 1024)     # d hb = dgrad(mu head) + dgrad(logvar head)
        dh = b.buf("g.dh", B * 1024)
        b.bn_bwd(bwd, h, dhb_a, dh, B, 1024, fc_bn, h_saved)
        # the factored multi-rank exchange and the one-rank outer-product Adam compute fc.0's weight gradient instead
        bwd.hook("fc_wgrad", replaces_next=True)
        b.lin_wgrad(bwd, dh, flat, grad_of(fc_lin.weight), B, 1024, F0)
        self._fc_factors = (dh, flat, fc_lin.weight, F0)
        b.lin_dgrad(bwd, dh, fc_lin.weight, gA, B, 1024, F0)
        # the encoder's dense gradients (fc.0 = 134 MB at config 3, fc.1, l_mu, l_var) are final and its dense
        # parameters are not read any more: second bucket
        bwd.hook("enc_dense_done")
        bwd.add("vp_nchw_to_nhwc_f32", P(gA), P(gB), B, size, 8, 8)
        cur, other = gB, gA
        # the encoder-tail bucket: its hook's index in the backward plan and the first of the blocks it covers (None: no such bucket)
        self._bwd_b_enc_tail = self._enc_tail_first = None
        for i in range(L - 1, -1, -1):
            blk, Cin, Cout, Hs, p1, c, saved = enc_rec[i]
            R = B * Hs * Hs
            fl = 50.0 * B * Hs * Hs * Cin * Cout
            geom = (B, Hs, Hs, Cin, Cout, 2)
            if i == 0 and enc0_cols:
                xcol, KC = enc0
                k, gS = b.next_plane(bwd)
                b.bn_bwd(bwd, c, cur, None, R, Cout, blk.bn, saved, gS)  # gS = d c_0 (split)
                dwc = b.buf("enc0.dwc", Cout * KC)
                ws0 = b.ws("enc0.wgws", lib.vp_conv_wgrad_bf16x3_workspace_bytes(B, Hs, Hs, Hs, Hs, KC, Cout, 1, 1))
                # the LAST weight gradient of the step stays on the main stream: on the side stream the join that follows it (and
                # precedes the optimiser) finds both queues idle for ~18 us -- the latency of a dependency between two hardware
                # queues (profiles/r02_notes.md) -- while here the side stream has long finished when the main stream joins it
                if x2:
                    bwd.add("vp_conv_wgrad_f16x2", P(xcol), P(gS), P(dwc), B, Hs, Hs, Hs, Hs, KC, Cout, 1, 1, 1.0 / GS, P(ws0), ws0.numel() * 4,
                            flops=fl, tag="enc0.wgrad")
                else:
                    bwd.add("vp_conv_wgrad_bf16x3", P(xcol), P(gS), P(dwc), B, Hs, Hs, Hs, Hs, KC, Cout, 1, 1, P(ws0), ws0.numel() * 4,
                            flops=fl, tag="enc0.wgrad")
                bwd.add("vp_unpack_dw_im2col5_f32", P(dwc), P(grad_of(blk.conv.weight)), Cout, Cin)
            elif enc16[i]:
                k, gS = b.next_plane(bwd)
                b.bn_bwd(bwd, c, cur, None, R, Cout, blk.bn, saved, gS)  # gS = d c_i (split)
                b.wgrad5(bwd, enc_in_s[i], gS, grad_of(blk.conv.weight), geom, k, flops=fl, tag=f"enc{i}.wgrad")
                if i > 0:
                    b.conv5(bwd, 1, a16, gS, p1, cur, (B, Hs, Hs, Cout, Cin, 2), products=2, alpha=1.0 / GS,
                            flops=fl, tag=f"enc{i}.dgrad")                             # cur = d a_{i-1}
                if i == max(L - 2, 1):
                    # the gradients of encoder.conv[i:] (16.4 of the 17 MB of conv parameters at config 3) are issued: third bucket
                    self._bwd_b_enc_tail, self._enc_tail_first = len(bwd.calls), i
                    bwd.hook("enc_tail")
            elif i == 0 and enc0_cols32:
                xcol, KC = enc0
                b.bn_bwd(bwd, c, cur, other, R, Cout, blk.bn, saved)            # other = d c_0
                dwc = b.buf("enc0.dwc", Cout * KC)
                ws0 = b.ws("enc0.wgws", lib.vp_conv_wgrad_workspace_bytes(B, Hs, Hs, Hs, Hs, KC, Cout, 1, 1))
                bwd.add("vp_conv_wgrad_f32", P(xcol), P(other), P(dwc), B, Hs, Hs, Hs, Hs, KC, Cout, 1, 1, P(ws0), ws0.numel() * 4,
                        flops=fl, tag="enc0.wgrad")
                bwd.add("vp_unpack_dw_im2col5_f32", P(dwc), P(grad_of(blk.conv.weight)), Cout, Cin)
            else:
                b.bn_bwd(bwd, c, cur, other, R, Cout, blk.bn, saved)            # other = d c_i
                # side stream only for the last layer of the walk (i == 0): nothing rewrites `other` after it
                bwd.add("vp_conv5_wgrad_f32", P(enc_in[i]), P(other), P(grad_of(blk.conv.weight)), *geom,
                        P(ws_wg), ws_wg.numel() * 4, flops=fl, tag=f"enc{i}.wgrad", side=(b.side_slot() if i == 0 else None))
                if i > 0:
                    b.conv5(bwd, 1, "f32", other, p1, cur, (B, Hs, Hs, Cout, Cin, 2), flops=fl, tag=f"enc{i}.dgrad")  # cur = d a_{i-1}
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
        the sticky saturation flag of the fp16 gradient planes (a host sync, like everything here) and raises when a step since the
        last call clamped a gradient at +-65504 / grad_scale16 -- the weights of those steps are off; lower ``grad_scale16``."""
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
