"""Fused VAE-GAN training step (BASELINE config 4): the loop body of train.py:43-78 -- VaeGan.forward (models/networks.py:233-248),
VaeGan.loss (:264-281), the five losses of train.py:61-66, their five ``backward(retain_graph=True)`` calls and the four RMSprop
updates -- as ONE pre-planned sequence of HIP kernel launches on the ``_Plan`` machinery of engine.py: no autograd graph, no
per-step allocation, no ATen arithmetic on the path.

What the plan does differently from the autograd front end (functional.py), with identical arithmetic per kernel:
  * ONE backward traversal: train.py:69-73 accumulates the five losses' gradients into the same ``.grad`` tensors, i.e. every
    parameter receives the gradient of  recon + sum(kl) + (1 + lambda) sum(mse) + (1 - (1 - lambda)) loss_discriminator + l1;
    the two coefficients are formed in fp32 exactly as autograd's accumulation forms them;
  * ONE pass over the discriminator's conv stack for its "REC" and "GAN" calls (models/networks.py:244-245); the second
    running-statistics update of the blocks both calls run is replayed from the buffers (as Discriminator.forward_rec_and_gan);
  * convolution weights packed once per step for both decoder passes (z and z_p) by one batched launch on the side stream;
  * BatchNorm statistics from the convolution's epilogue, split-bf16 operand planes written by the BatchNorm kernels;
  * weight gradients on a side stream underneath the HBM-bound BatchNorm / elementwise kernels of the main chain;
  * every gradient written once, straight into the four optimisers' flat arenas (the decoder's second pass into a shadow arena
    that ONE add folds in); the arenas are then all-reduced (several ranks) and consumed by the fused RMSprop kernels.

Arithmetic: the 5x5 convolutions with channel counts that are multiples of 8 on the split-bf16 kernels ("bf16x3"), the image-side
convolutions on the edge MFMA kernels, dense layers on the exact-fp32 kernels -- the same kernels ``set_conv_precision("bf16x3")``
selects for the drop-in modules, so the step equals the autograd path (tests/test_gpu_engine_gan.py).
"""
from __future__ import annotations

import os
from ctypes import c_void_p
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, ops, parallel, sections
from .networks import VaeGan
from .plan import PlanBuilder, _Plan, _ptr, grad_of, plan_device, side_ctx, sync_counters_on_state_dict

_ACT_RELU, _ACT_NONE, _ACT_SIGMOID = ops.ACT_RELU, ops.ACT_NONE, ops.ACT_SIGMOID


class FusedVAEGANStep:
    """forward + losses + backward (+ all-reduce + the four RMSprop updates) for a ``networks.VaeGan``.

    ``optimizers`` = flat-arena optimisers (vae_play_amd.optim) over net.encoder / net.decoder / net.discriminator /
    net.param_encoder parameters, in any order (train.py:212-219 builds exactly these four); every parameter must live in one
    of their arenas, the decoder's in a single one."""

    def __init__(self, net: VaeGan, optimizers, batch_size: int, img_size: int, lambda_mse: float = 1e-6, group=None,
                 _plan_only: bool = False):
        self.net, self.opts, self.B, self.S = net, list(optimizers), int(batch_size), int(img_size)
        self.Z, self.L = net.z_size, net.iter_level
        self.lam = float(lambda_mse)
        self.group = group
        self.world = torch.distributed.get_world_size(group) if torch.distributed.is_initialized() else 1
        for o in self.opts:
            o.grad_scale = 1.0 / self.world
        dev = plan_device(net, "FusedVAEGANStep", _plan_only)   # (_plan_only: the launch list over host buffers, for tests)
        if self.S != 8 * 2 ** self.L:
            raise ValueError("img_size must be 8 * 2**iter_level")
        if net.discriminator.recon_levl != len(net.discriminator.conv) - 1:
            raise NotImplementedError("the fused plan taps the discriminator's last block (VaeGan's own construction)")
        for p in net.parameters():
            if getattr(p, "_vp_arena", None) is None:
                raise _lib.VaePlayHipError("every VaeGan parameter must live in a flat-arena optimiser")
        self.dev = dev
        self._bufs: Dict[str, torch.Tensor] = {}
        self._steps_since_sync = 0
        self._build()
        self._sd_hook = sync_counters_on_state_dict(self, net)

    # ---- plan construction ------------------------------------------------------------------
    def _build(self):
        B, S, Z, L = self.B, self.S, self.Z, self.L
        net = self.net
        enc, dec, disc, pe = net.encoder, net.decoder, net.discriminator, net.param_encoder
        env = os.environ.get
        P = _ptr
        fwd, fwd_disc, bwd = _Plan(), _Plan(), _Plan()
        n3 = 3 * B
        n_pix = B * S * S
        # CU budget of a weight gradient beside the main stream's kernels (csrc/wgrad5.h; 128 / 192 / 256: 5.78 / 5.91 / 6.04 ms)
        b = PlanBuilder(self, self.dev, "bf16x3", side_on=env("VP_SIDE_WGRAD", "1") != "0",
                        wgrad_cus=(0, int(env("VP_WGRAD_SIDE_CUS", "128"))), fuse_stats=env("VP_FUSE_BN_STATS", "1") != "0")
        lib = b.lib

        def at(t: torch.Tensor, off_elems: int):
            return c_void_p(t.data_ptr() + 4 * off_elems)

        dec_arena = next(dec.parameters())._vp_arena
        if any(p._vp_arena is not dec_arena for p in dec.parameters()):
            raise _lib.VaePlayHipError("the decoder's parameters must live in one arena")
        self._dec_arena = dec_arena
        self._dec_shadow = torch.zeros_like(dec_arena.flat_grad)
        # optimisers whose arena holds exactly one sub-network's parameters (train.py:212-219 builds one optimiser per sub-network):
        # candidates for an early update; an arena shared between sub-networks is updated at the end of the step
        self._arena_opts = {"disc": [], "dec": []}
        for kind, mod in (("disc", net.discriminator), ("dec", dec)):
            ids = {id(p) for p in mod.parameters()}
            for o in self.opts:
                if o.arena.numel and {id(p) for p in o.arena.params} == ids and not getattr(o.arena, "foreign", None):
                    self._arena_opts[kind].append(o)
        self._early_done = set()
        # the encoder's arena: conv blocks first, then fc.0 / fc.1 / l_mu / l_var (Encoder's parameter order); the dense slice -- 90 % of
        # it -- can be updated as soon as the dense backward is through, the conv slice only at the end of the step
        self._enc_dense = []
        enc_ids = {id(p) for p in enc.parameters()}
        conv_ids = {id(p) for p in enc.conv.parameters()}
        for o in self.opts:
            a = o.arena
            if a.numel and {id(p) for p in a.params} == enc_ids and not getattr(a, "foreign", None):
                lo = min(off for p, off in zip(a.params, a.offsets) if id(p) not in conv_ids)
                if all((id(p) in conv_ids) == (off < lo) for p, off in zip(a.params, a.offsets)):
                    self._enc_dense.append((o, lo))
        self._early_partial = {}

        def grad2_of(p):         # second decoder pass: same offsets in the shadow arena
            return self._dec_shadow[p._vp_off:p._vp_off + p.numel()].view_as(p)

        def require16(blocks, what):
            # (the sections would route other widths to the fp32 kernels: a combination this step has never run)
            if not all(k.is16 for k in blocks):
                raise NotImplementedError(f"{what} widths must be multiples of 8")

        # =================================================== forward ===================================================
        self.xcat = b.buf("xcat", n3, 1, S, S)        # (original | reconstructed | sampled): the discriminator's batch
        self.eps, self.z_p = b.buf("eps", B, Z), b.buf("z_p", B, Z)
        self.targets = b.buf("targets", B, 3)
        xcat = self.xcat

        # ---- encoder (models/networks.py:49-78): im2col stem over xcat[:B], gather blocks, head ----
        if enc.conv[0].conv.weight.shape[0] % 8:
            raise NotImplementedError("encoder width must be a multiple of 8")
        enc_blocks = sections.gather_stack(b, "enc", enc.conv, B, S, None, None, image=xcat)
        require16(enc_blocks, "encoder")
        for i, blk in enumerate(enc_blocks):
            if i == 1 and b.k_pack is not None:
                fwd.wait_side(b.k_pack)
            blk.fwd(fwd)
        if L == 1 and b.k_pack is not None:
            fwd.wait_side(b.k_pack)
        head = sections.EncoderHead(b, enc, B, enc_blocks[-1].Cout)
        head.fwd(fwd, enc_blocks[-1].a)
        head.latent(fwd, self.eps)
        self.mu, self.logvar, self.z, self.kl = head.mu, head.logvar, head.z, head.kl

        # ---- decoder (models/networks.py:81-112), run on z and on z_p with the same packed weights ----
        # (own_wgrad_ws, halo_dgrad: kept so that this plan's buffers and launches stay as they are)
        trunk = sections.DecoderTrunk(b, dec, B, L, S, 1, own_wgrad_ws=True, halo_dgrad=False)
        if any(ch % 8 for ch in trunk.ch):
            raise NotImplementedError("decoder widths must be multiples of 8")
        Cf = trunk.ch[-1]
        dec1 = trunk.fwd(fwd, "dec", self.z, at(xcat, n_pix), "dec.fin")            # x_tilde = xcat[B:2B]

        # ---- param_encoder (DirectDecoder, models/networks.py:118-148): bias-ed Linear layers without activations ----
        pe_rec = []

        def pe_lin(tag, lin, x):
            N, K = lin.weight.shape
            y = b.buf(f"pe.{tag}", B * N)
            b.lin_fwd(fwd, x, lin.weight, lin.bias, y, B, N, K)
            pe_rec.append((tag, lin, x, y, N, K))
            return y
        t_ = self.z
        for j, lin in enumerate(pe.head):
            t_ = pe_lin(f"head{j}", lin, t_)
        pe_head = t_
        self.p_r = pe_lin("r1", pe.r_fc[1], pe_lin("r0", pe.r_fc[0], pe_head))
        self.p_xy = pe_lin("xy1", pe.xy_fc[1], pe_lin("xy0", pe.xy_fc[0], pe_head))
        n_r, n_xy = pe.r_fc[1].weight.shape[0], pe.xy_fc[1].weight.shape[0]
        if n_r + n_xy != self.targets.shape[1]:
            raise ValueError("targets must have as many columns as DirectDecoder returns")
        self.l1 = b.buf("l1", 1)
        d_r, d_xy = b.buf("g.d_r", B * n_r), b.buf("g.d_xy", B * n_xy)
        fwd.add("vp_smooth_l1_cat_f32", P(self.targets), P(self.p_r), P(self.p_xy), B, n_r, n_xy, 1.0 / B, P(self.l1), P(d_r), P(d_xy))

        dec2 = trunk.fwd(fwd, "decp", self.z_p, at(xcat, 2 * n_pix), "decp.fin")    # x_p = xcat[2B:3B]

        # ---- discriminator on (x | x_tilde | x_p) (models/networks.py:151-198), one pass for "REC" and "GAN" ----
        conv0 = disc.conv[0][0]
        C0 = conv0.weight.shape[0]
        if C0 not in (32, 64) or conv0.weight.shape[1] != 1:
            raise NotImplementedError("discriminator stem must be 1 -> 32 | 64 channels")
        y0 = b.buf("disc0.y", n3 * S * S * C0)
        y0s = b.sbuf("disc0.ys", n3 * S * S * C0)
        fwd_disc.add("vp_conv5_smallin_fwd_bf16x3", P(xcat), P(conv0.weight), P(conv0.bias), P(y0), n3, S, S, 1, C0, _ACT_RELU,
                     flops=50.0 * n3 * S * S * C0, tag="disc0.fwd")
        fwd_disc.add("vp_split_f32", P(y0), P(y0s), n3 * S * S * C0)
        # (count=2: the reference runs these blocks twice per step)
        disc_blocks = sections.gather_stack(b, "disc", list(disc.conv)[1:], n3, S, None, y0s, count=2, first_index=1)
        require16(disc_blocks, "discriminator")
        for blk in disc_blocks:
            blk.fwd(fwd_disc)
        self._disc_replay = [blk.bn for blk in disc_blocks]
        last = disc_blocks[-1]
        Cd = last.Cout
        nf = 64 * Cd                                               # features per image at the tap
        tap = last.c                                               # pre-BatchNorm output of the last block: "disc_layer"
        dflat = b.buf("disc.flat", n3 * nf)
        fwd_disc.add("vp_nhwc_to_nchw_f32", P(last.a), P(dflat), n3, Cd, 8, 8)
        dl0, dl_bn, dl3 = disc.fc[0], disc.fc[1], disc.fc[3]
        Hd = dl0.weight.shape[0]
        dh, dhb = b.buf("disc.h", n3 * Hd), b.buf("disc.hb", n3 * Hd)
        b.lin_fwd(fwd_disc, dflat, dl0.weight, None, dh, n3, Hd, nf)
        dh_saved = b.bn_fwd(fwd_disc, "disc.fc", dh, n3, Hd, dl_bn, dhb)
        logit = b.buf("disc.logit", n3)
        b.lin_fwd(fwd_disc, dhb, dl3.weight, dl3.bias, logit, n3, 1, Hd)
        # coefficients of the summed losses, formed in fp32 as autograd's accumulation forms them (train.py:63-66)
        one = np.float32(1.0)
        self.c_disc = float(one + (-np.float32(1.0 - self.lam)))          # loss_discriminator: 1 from itself, -(1 - lambda) from loss_decoder
        self.c_mse = float(one + np.float32(self.lam))                    # sum(mse): 1 from loss_encoder, lambda from loss_decoder
        self.disc_class = b.buf("disc_class", n3, 1)
        self.bce_sums = b.buf("bce_sums", 3)
        dlogit = b.buf("g.dlogit", n3)
        fwd_disc.add("vp_gan_head_f32", P(logit), B, self.c_disc, P(self.disc_class), P(self.bce_sums), P(dlogit))
        self.mse = b.buf("mse", B)
        fwd_disc.add("vp_half_sqdiff_rowsum_f32", P(tap), at(tap, B * nf), P(self.mse), B, nf)
        self.nle_rows = b.buf("nle_rows", B)                   # sum over pixels of "nle" (models/networks.py:267) per image
        fwd_disc.add("vp_half_sqdiff_rowsum_f32", P(xcat), at(xcat, n_pix), P(self.nle_rows), B, S * S)
        self.disc_layer_nhwc = tap.view(n3, 8, 8, Cd)

        # =================================================== backward ===================================================
        dec_acts = [B * 4 * Hs * Hs * Cout for Hs, _, Cout in trunk.layers]
        big_d = max([n3 * S * S * C0] + [k.R * k.Cout for k in disc_blocks] + [n3 * nf])
        big_v = max([B * head.F0, B * trunk.F1, n_pix * Cf] + dec_acts + [k.R * k.Cout for k in enc_blocks])
        gA, gB = b.buf("g.A", big_d), b.buf("g.B", big_d)          # discriminator phase
        hA, hB = b.buf("g.hA", big_v), b.buf("g.hB", big_v)        # decoder / encoder phases
        b.grad_planes(max([k.R * k.Cout for k in disc_blocks + enc_blocks] + dec_acts))
        b.wgrad_workspace([(k.Bn, k.Hs, k.Cin, k.Cout) for k in disc_blocks + enc_blocks[1:]]
                          + [(B, Hs, Cout, Cin) for Hs, Cin, Cout in trunk.layers])

        # ---- discriminator head ----
        b.lin_wgrad(bwd, dlogit, dhb, grad_of(dl3.weight), n3, 1, Hd)
        b.colsum(bwd, "disc.b3", dlogit, grad_of(dl3.bias), n3, 1)
        g_hb, g_h = b.buf("g.disc_hb", n3 * Hd), b.buf("g.disc_h", n3 * Hd)
        b.lin_dgrad(bwd, dlogit, dl3.weight, g_hb, n3, 1, Hd)
        b.bn_bwd(bwd, dh, g_hb, g_h, n3, Hd, dl_bn, dh_saved)
        b.lin_wgrad(bwd, g_h, dflat, grad_of(dl0.weight), n3, Hd, nf)
        b.lin_dgrad(bwd, g_h, dl0.weight, gA, n3, Hd, nf)
        bwd.add("vp_nchw_to_nhwc_f32", P(gA), P(gB), n3, Cd, 8, 8)         # gB = d (last block's activation)
        # ---- last block: its pre-BatchNorm output also feeds the feature loss (1 + lambda) * sum(mse) ----
        g_mse = b.buf("g.c_mse", B).fill_(self.c_mse)
        m_ab = b.buf("g.mse_ab", 2 * B * nf)

        def tap_split(gS):
            b.bn_bwd(bwd, tap, gB, gA, last.R, last.Cout, last.bn, last.saved)                          # gA = BatchNorm path
            bwd.add("vp_half_sqdiff_bwd_f32", P(tap), at(tap, B * nf), P(g_mse), P(m_ab), at(m_ab, B * nf), B, nf, 1)
            bwd.add("vp_add_f32", P(gA), P(m_ab), P(gA), 2 * B * nf)                              # + feature loss (original, reconstructed)
            bwd.add("vp_split_f32", P(gA), P(gS), n3 * nf)
        last.bwd(bwd, gB, gA, pre_split=tap_split)
        for blk in reversed(disc_blocks[:-1]):
            blk.bwd(bwd, gB, gA)
        # ---- stem: conv 1 -> C0 + bias + ReLU (ReLU in the convolution's epilogue) ----
        n0 = n3 * S * S * C0
        bwd.add("vp_act_bwd_from_y_f32", P(y0), P(gB), P(gA), n0, _ACT_RELU, 0.0)                  # gA = d (conv output)
        k_stem = b.side_slot()
        b.colsum(bwd, "disc.b0", gA, grad_of(conv0.bias), n3 * S * S, C0, side=b.side_slot())
        ws_w0 = b.ws("disc0.wgws", lib.vp_conv5_wgrad_workspace_bytes(n3, S, S, 1, C0, 1))
        bwd.add("vp_conv5_wgrad_f32", P(xcat), P(gA), P(grad_of(conv0.weight)), n3, S, S, 1, C0, 1, P(ws_w0), ws_w0.numel() * 4,
                flops=50.0 * n3 * S * S * C0, tag="disc0.wgrad", side=k_stem)
        self._wf = b.buf("disc0.wf", 25 * C0)                   # taps flipped, [ci = 1][tap][co]: the input gradient is a correlation
        self._conv0_w = conv0.weight
        dxc = b.buf("g.dxcat", 2 * n_pix)                       # d x_tilde | d x_p from the discriminator
        bwd.add("vp_conv5_smallout_bf16x3", at(gA, B * S * S * C0), P(self._wf), None, P(dxc), 2 * B, S, S, C0, 1, _ACT_NONE,
                flops=50.0 * 2 * B * S * S * C0, tag="disc0.dgrad")
        bwd.hook("disc_done")       # every discriminator gradient is launched and none of its parameters is read again in this step

        # ---- decoder ----
        def dec_bwd(ps, dout, gfn, dz):
            """``dout`` = pointer to the gradient w.r.t. the sigmoid output (fp32, B*S*S); writes d z into ``dz`` when given"""
            dlg = b.buf(f"g.{ps.tag}.dlogit", n_pix)
            bwd.add("vp_act_bwd_from_y_f32", ps.out, dout, P(dlg), n_pix, _ACT_SIGMOID, 0.0)
            trunk.bwd(bwd, ps, dlg, hA, hB, gfn, dz)

        # second pass first (x_p: only the discriminator's gradient reaches it), into the shadow arena
        dec_bwd(dec2, at(dxc, n_pix), grad2_of, None)

        # ---- param_encoder ----
        pe_by = {r[0]: r for r in pe_rec}

        def pe_bwd(tag, dy):
            _, lin, x, y, N, K = pe_by[tag]
            b.lin_wgrad(bwd, dy, x, grad_of(lin.weight), B, N, K)
            b.colsum(bwd, f"pe.{tag}", dy, grad_of(lin.bias), B, N)
            dx = b.buf(f"g.pe.{tag}.dx", B * K)
            b.lin_dgrad(bwd, dy, lin.weight, dx, B, N, K)
            return dx
        d_head_a = pe_bwd("r0", pe_bwd("r1", d_r))
        d_head_b = pe_bwd("xy0", pe_bwd("xy1", d_xy))
        bwd.add("vp_add_f32", P(d_head_a), P(d_head_b), P(d_head_a), d_head_a.numel())
        dz_pe = d_head_a
        for j in range(len(pe.head) - 1, -1, -1):
            dz_pe = pe_bwd(f"head{j}", dz_pe)
        # ---- first decoder pass: d x_tilde = discriminator part + reconstruction loss mean((x - x_tilde)^2) (train.py:61) ----
        g_rec = b.buf("g.c_rec", 1).fill_(2.0 / n_pix)
        dxt = b.buf("g.dxt", n_pix)
        bwd.add("vp_half_sqdiff_bwd_f32", P(xcat), at(xcat, n_pix), P(g_rec), None, P(dxt), 1, n_pix, 1)     # 2/n (x_tilde - x)
        bwd.add("vp_add_f32", P(dxt), P(dxc), P(dxt), n_pix)
        dz_dec = b.buf("g.dz_dec", B * Z)
        dec_bwd(dec1, P(dxt), grad_of, dz_dec)
        bwd.hook("dec_done")        # both decoder passes' gradients are launched; the decoder's parameters are not read again
        dz = b.buf("g.dz", B * Z)
        bwd.add("vp_add_f32", P(dz_dec), P(dz_pe), P(dz), B * Z)

        # ---- encoder: head (the KL term is not averaged over the batch here), gather blocks, stem ----
        head.bwd(bwd, self.eps, dz, 1.0, hA, hB)
        for blk in reversed(enc_blocks):
            blk.bwd(bwd, hB, hA)

        b.finish(fwd)
        self._fwd, self._fwd_disc, self._bwd = fwd, fwd_disc, bwd
        self._bn_counts = b.bn_counts              # (BatchNormAct module, forward passes per step)
        self._snap = [torch.empty_like(bn.running_mean) for bn in self._disc_replay] + [torch.empty_like(bn.running_var) for bn in self._disc_replay]
        self._running = [bn.running_mean for bn in self._disc_replay] + [bn.running_var for bn in self._disc_replay]
        self.x_tilde = xcat[B:2 * B]
        self.x_p = xcat[2 * B:]

    # ---- execution ---------------------------------------------------------------------------
    def _side_ctx(self):
        return side_ctx(self)

    @torch.no_grad()
    def forward_backward(self, x: torch.Tensor, targets: torch.Tensor, eps: torch.Tensor, z_p: torch.Tensor, timers: Optional[dict] = None,
                         early_updates: bool = False):
        """Gradients of the summed losses of train.py:61-73 land in the four optimisers' flat gradient arenas.  ``eps`` is the
        reparameterisation noise (models/networks.py:230), ``z_p`` the prior sample (:240).  Outputs (static buffers, overwritten
        by the next step): ``x_tilde``, ``x_p``, ``mu``, ``logvar``, ``disc_class``, ``kl``, ``mse``, ``bce_sums``, ``l1``,
        ``nle_rows``; ``losses()`` assembles train.py's five scalars from them."""
        B = self.B
        self.xcat[:B].copy_(x.reshape(B, 1, self.S, self.S), non_blocking=True)
        self.targets.copy_(targets, non_blocking=True)
        self.eps.copy_(eps, non_blocking=True)
        self.z_p.copy_(z_p, non_blocking=True)
        w = self._conv0_w.detach()
        self._wf.view(1, 25, -1).copy_(w.flip(2, 3).permute(1, 2, 3, 0).reshape(1, 25, -1))
        s = torch.cuda.current_stream().cuda_stream
        side = self._side_ctx() if timers is None else None
        self._fwd.run(s, timers, side=side)
        # the reference runs the discriminator twice per step: the blocks' running statistics move twice (second update replayed
        # from the buffers before / after the single pass: rm2 = (2 - m) rm1 - (1 - m) rm0)
        torch._foreach_copy_(self._snap, self._running)
        self._fwd_disc.run(s, timers, side=side)
        m = float(self._disc_replay[0].momentum)
        torch._foreach_mul_(self._running, 2.0 - m)
        torch._foreach_add_(self._running, self._snap, alpha=-(1.0 - m))
        self._early_done = set()
        self._early_partial = {}
        hooks = None
        if early_updates and side is not None:
            # RMSprop of an arena as soon as its gradients are launched, ON THE SIDE STREAM (behind that arena's weight gradients, which
            # run there; the fork covers the gradients the main stream produced): HBM-bound updates underneath the MFMA-bound backward
            # of the networks that are still to come instead of behind the whole step
            def early(kind):
                def fn(sd):
                    if not self._arena_opts[kind]:          # (an arena shared between sub-networks: updated at the end of the step)
                        return

                    def update():
                        if kind == "dec":
                            a = self._dec_arena
                            _lib.call("vp_add_f32", _ptr(a.flat_grad), _ptr(self._dec_shadow), _ptr(a.flat_grad), a.flat_grad.numel(),
                                      c_void_p(sd.stream.cuda_stream))
                        for o in self._arena_opts[kind]:
                            o.begin_step()
                            o.step_range(0, o.arena.flat_param.numel())
                            self._early_done.add(id(o))
                    sd.run(update)
                return fn

            def early_enc_dense(sd):
                def update():
                    for o, lo in self._enc_dense:
                        o.begin_step()
                        o.step_range(lo, o.arena.flat_param.numel())
                        self._early_partial[id(o)] = lo
                if self._enc_dense:
                    sd.run(update)
            hooks = {"disc_done": early("disc"), "dec_done": early("dec"), "enc_dense_done": early_enc_dense}
        self._bwd.run(s, timers, side=side, hooks=hooks)
        if side is not None:
            side.join()
        if not any(id(o) in self._early_done for o in self._arena_opts["dec"]):
            a = self._dec_arena
            _lib.call("vp_add_f32", _ptr(a.flat_grad), _ptr(self._dec_shadow), _ptr(a.flat_grad), a.flat_grad.numel(), c_void_p(s))
        for o in self.opts:        # the plan wrote the arenas: a ``.grad`` left None by module.zero_grad() must not read as "no gradient"
            o.arena.adopt_views()
        self._steps_since_sync += 1

    def step(self, x, targets, eps, z_p, timers: Optional[dict] = None):
        """One training iteration of train.py:43-78: forward, losses, backward, gradient all-reduce (several ranks), four RMSprop updates."""
        early = (not parallel.dp_active(self.group)) and timers is None and os.environ.get("VP_GAN_EARLY_UPDATES", "1") != "0"
        self.forward_backward(x, targets, eps, z_p, timers, early_updates=early)
        arenas = []
        for o in self.opts:
            if o.arena.numel and all(o.arena is not q for q in arenas):
                arenas.append(o.arena)
        if parallel.dp_active(self.group):
            works = [parallel.allreduce_flat_grads(a.flat_grad, self.group, async_op=True) for a in arenas]
            for w in works:
                if w is not None:
                    w.wait()
        for o in self.opts:
            if id(o) in self._early_done:      # updated on the side stream during backward (forward_backward's hooks)
                continue
            if id(o) in self._early_partial:   # its dense slice was: the rest now, same step count
                o.step_range(0, self._early_partial[id(o)])
                continue
            o.begin_step()
            o.step_range(0, o.arena.flat_param.numel() if o.arena.numel else 0)

    def losses(self) -> dict:
        """train.py:61-66's scalars from the last step's buffers (host arithmetic on a handful of device scalars; a sync)."""
        kl, mse = float(self.kl.sum()), float(self.mse.sum())
        d = float(self.bce_sums.sum())
        n = self.B * self.S * self.S
        return {"loss_recon": 2.0 * float(self.nle_rows.sum()) / n, "loss_encoder": kl + mse, "loss_discriminator": d,
                "loss_decoder": self.lam * mse - (1.0 - self.lam) * d, "loss_aux": float(self.l1)}

    @property
    def params(self) -> torch.Tensor:
        """DirectDecoder's output cat([r, xy], -1) of the last step"""
        return torch.cat([self.p_r.view(self.B, -1), self.p_xy.view(self.B, -1)], dim=-1)

    @property
    def disc_layer(self) -> torch.Tensor:
        """the "REC" output of the last step in the reference's (C, H, W) flatten order, (3B, C*8*8)"""
        return self.disc_layer_nhwc.permute(0, 3, 1, 2).reshape(3 * self.B, -1)

    def sync_counters(self):
        """Advance BatchNorm ``num_batches_tracked`` buffers (bookkeeping only; kept off the hot path)."""
        n = self._steps_since_sync
        if n:
            for bn, count in self._bn_counts:
                bn.num_batches_tracked.add_(n * count)
            self._steps_since_sync = 0
