"""Fused VAE inference: encode / decode / reconstruct / sample of a trained model as fixed, pre-planned lists of HIP launches
(no autograd, no per-call allocation, hipGraph-replayable), with every eval-mode BatchNorm of a convolution block folded into
that convolution's epilogue.

In eval mode BatchNorm is the per-channel affine map y = s x + t, s = gamma / sqrt(running_var + eps), t = beta - running_mean s,
known before the launch.  A block (5x5 convolution -> BatchNorm -> ReLU) is therefore ONE launch here: the implicit-GEMM kernel
applies act(fma(acc, s, t)) to its accumulators and writes the next layer's operand -- split bf16 planes, or fp32 -- directly
(csrc/igemm16.h ``epilogue_affine32``), where the module path writes the fp32 convolution output and reads it back in a separate
normalise pass.  Launch shapes the library does not fuse (``vp_conv5_affine_supported() == 0``: the few-tile layers whose plain
launch splits K, and the first encoder block on its im2col) keep convolution + one normalise pass.

Reference paths replaced: the ``eval()`` branch of VaeGan.forward (models/networks.py:248-258: sample and decode; encode ->
reparameterise -> decode), the ``torch.no_grad()`` reconstruction inside the training loop (train.py:95-96), and the plain-VAE
composition of Encoder (models/networks.py:72-78), reparameterize (:228-231) and Decoder (:107-112).

``score`` adds what validation, model comparison and anomaly scoring need: per image the reconstruction term (the reference's
per-pixel ``F.binary_cross_entropy``, summed over the image), the KL term (models/networks.py:270), their sum (the ELBO) and the
K-sample importance-weighted bound.  The reference has no evaluation loop with a loss; the importance-weighted bound is new
functionality, not a port.  It reuses the launches above -- encode once, decode K times -- plus the three kernels of csrc/score.hip.

``project`` / ``decode_grad`` search the latent space for a given image: the gradient of the (optionally pixel-masked) reconstruction
term with respect to z through the frozen eval-mode decoder, and Adam on z with a Gaussian prior -- inversion, and with a mask
inpainting and occlusion-robust anomaly scoring.  Like the importance-weighted bound it has no counterpart in the reference: new
functionality, not a port.  One iteration is the decode list, three kernels of csrc/project.hip and the training plans' input-gradient
convolutions, as one replayable launch list.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional

import torch

from . import _lib, ops, sections
from .plan import PlanBuilder, _Plan, _ptr, plan_device


class FusedVAEInference:
    """encode / decode / reconstruct / sample / score for a ``networks.VAE`` (or an Encoder / Decoder pair: ``from_modules``).

    The plan SNAPSHOTS the model when it is built: convolution weights are packed into plan-owned buffers and every BatchNorm's
    running statistics and affine parameters are folded into plan-owned scale / shift / rstd vectors, once, not per call.  After the
    module's parameters or buffers change (training continued, ``load_state_dict``) call ``refresh()``; until then the plan keeps
    computing with the weights it was built with -- a stale plan does NOT pick the changes up.  (Dense-layer weights, biases and the
    dense BatchNorms' running means are read in place, so a stale plan after a change is neither the old nor the new model:
    always ``refresh()``.)  Nothing here writes to the module: parameters, running statistics, ``num_batches_tracked`` and the
    ``training`` flags are never modified, and the result is eval-mode arithmetic whatever ``module.training`` says.

    ``precision``: "bf16x3" (5x5 layers on split-bf16 operands, three MFMAs per product), "f32" (exact fp32 products) or "f16"
    (one product: activations and weights of the 5x5 blocks rounded to fp16 -- 11 significant bits, saturating at +-65504 -- and
    contracted with ONE fp16 MFMA per fragment pair and fp32 accumulation; the final convolution and the dense layers keep the
    bf16x3 plan's kernels.  Inference only: the training plans have no such mode.  Measured errors and throughput: DESIGN.md 14.2).
    Inputs of any number of rows run in chunks of ``batch_size``; a short last chunk is padded with zero rows (eval-mode rows are
    independent).  Module I/O is logical NCHW fp32."""

    def __init__(self, vae, batch_size: int, img_size: int, channels: int, precision: str = "bf16x3", _plan_only: bool = False):
        self._init(vae.encoder, vae.decoder, batch_size, img_size, channels, precision, _plan_only)

    @classmethod
    def from_modules(cls, encoder, decoder, batch_size: int, img_size: int, channels: int = 1, precision: str = "bf16x3",
                     _plan_only: bool = False) -> "FusedVAEInference":
        """the same over an ``Encoder`` / ``Decoder`` pair, e.g. the two halves of a ``networks.VaeGan`` (``channels = 1``)"""
        self = cls.__new__(cls)
        self._init(encoder, decoder, batch_size, img_size, channels, precision, _plan_only)
        return self

    def _init(self, encoder, decoder, batch_size, img_size, channels, precision, plan_only):
        if precision not in ("bf16x3", "f32", "f16"):
            raise ValueError("precision must be 'bf16x3', 'f32' or 'f16'")
        if batch_size <= 0 or img_size < 16 or img_size & (img_size - 1):
            raise ValueError("batch_size must be positive and img_size a power of two >= 16")
        self.encoder, self.decoder, self.precision = encoder, decoder, precision
        self.B, self.S, self.C = int(batch_size), int(img_size), int(channels)
        self.Z, self.L = encoder.l_mu.out_features, len(encoder.conv)
        if encoder.conv[0].conv.weight.shape[1] != self.C or decoder.conv[self.L][0].weight.shape[0] != self.C:
            raise ValueError(f"the model does not take {self.C}-channel images")
        if self.S != 8 * 2 ** self.L or len(decoder.conv) != self.L + 1:
            raise ValueError(f"the model's {self.L} blocks do not fit {self.S}x{self.S} images")
        self.dev = plan_device(encoder, "FusedVAEInference", plan_only)
        self._bufs: Dict[str, torch.Tensor] = {}
        self._graphs: Dict[str, "torch.cuda.CUDAGraph"] = {}
        self._score: Optional[SimpleNamespace] = None       # the scoring buffers: none until enable_scoring() / the first score()
        self._proj: Optional[SimpleNamespace] = None        # the projection buffers and lists: none until enable_projection()
        self._build()
        if not plan_only:
            self.refresh()

    # ---- plan construction ------------------------------------------------------------------
    def _build(self):
        B, S, C, Z, L = self.B, self.S, self.C, self.Z, self.L
        enc, dec = self.encoder, self.decoder
        prep, p_enc, p_lat, p_dec = _Plan(), _Plan(), _Plan(), _Plan()
        P = _ptr
        b = PlanBuilder(self, self.dev, self.precision, side_on=False, wgrad_cus=(0, 0))

        # ---------------- encoder: stem / gather blocks in eval form -> head ----------------
        self.x_nchw = b.buf("x_nchw", B, C, S, S)
        self.eps = b.buf("eps", B, Z)
        first = enc.conv[0].conv.weight
        if C > 1 and not sections.Im2colStem.applies(b, C, first.shape[0]):
            x_nhwc = b.buf("x_nhwc", B * S * S * C)
            p_enc.add("vp_nchw_to_nhwc_f32", P(self.x_nchw), P(x_nhwc), B, C, S, S)
        else:
            x_nhwc = self.x_nchw          # one channel: the same memory order (the im2col kernels read NCHW themselves)
        blocks = sections.gather_stack(b, "enc", enc.conv, B, S, x_nhwc, None, image=self.x_nchw, train=False)
        for blk in blocks:
            blk.fwd_eval(p_enc, prep)
        head = sections.EncoderHead(b, enc, B, blocks[-1].Cout)
        head.fwd(p_enc, blocks[-1].a, prep)
        self.mu, self.logvar, self.z = head.mu, head.logvar, head.z

        # ---------------- latent: z = eps * exp(logvar / 2) + mu ----------------
        head.latent(p_lat, self.eps, kl=False)

        # ---------------- decoder: trunk in eval form ----------------
        trunk = sections.DecoderTrunk(b, dec, B, L, S, C, train=False)
        xt_nhwc = b.buf("xt_nhwc", B * S * S * C)
        dec_pass = trunk.fwd(p_dec, "dec", self.z, xt_nhwc, "fin", prep)
        # a block is ONE launch where the library fuses the folded BatchNorm into the convolution's epilogue
        self.fused_layers = [k.tag for k in blocks + dec_pass.blocks if k.fused]
        self.unfused_layers = [k.tag for k in blocks + dec_pass.blocks if not k.fused]
        if C > 1:
            self.x_tilde = b.buf("x_tilde", B, C, S, S)
            p_dec.add("vp_nhwc_to_nchw_f32", P(xt_nhwc), P(self.x_tilde), B, C, S, S)
        else:
            self.x_tilde = xt_nhwc.view(B, C, S, S)
        b.finish(prep)      # the batched weight re-pack at the head of ``prep``; the dense layers' workspace
        self._prep = prep
        self._trunk, self._dec_pass, self._xt_nhwc = trunk, dec_pass, xt_nhwc       # what enable_projection() differentiates
        self._plans = {"encode": (p_enc,), "decode": (p_dec,), "reconstruct": (p_enc, p_lat, p_dec)}

    # ---- execution ---------------------------------------------------------------------------
    def refresh(self) -> None:
        """Re-read the model: pack the convolution weights and fold every BatchNorm's running statistics and affine parameters into
        the plan's constants (and, once projection is enabled, its input-gradient packs; Adam's state is left alone).  Runs when the
        plan is built; call it again after the module's parameters or buffers changed.
        Graphs captured before are captured again: they replay the same buffers and would see the new constants, but replays of a
        graph instantiated BEFORE the eager re-pack launches were observed to go wrong on MI355X / ROCm (the split-K layer's
        memset + atomic-add pair produced garbage, deterministically, while the eager list stayed right)."""
        self._prep.run(torch.cuda.current_stream().cuda_stream)
        if self._proj is not None:
            self._proj.prep.run(torch.cuda.current_stream().cuda_stream)      # the projection's own packs; nothing else of it is reset
        if self._graphs:
            self._graphs = {}
            self.capture()

    def _run(self, which: str) -> None:
        g = self._graphs.get(which)
        if g is not None:
            g.replay()
            return
        s = torch.cuda.current_stream().cuda_stream
        for plan in self._plans[which]:
            plan.run(s)

    def capture(self, warmup: int = 2):
        """Capture encode, decode and reconstruct -- and the scoring and projection lists built so far (``score``, ``project``) --
        into one hipGraph each (linear launch lists, no allocation) and replay them from then on; the results are bit-identical to
        the eager launches.  A scoring or projection list first used after this is captured when it is built."""
        self._graphs = self._capture(list(self._plans), warmup)
        return self._graphs

    def _capture(self, names, warmup: int = 2):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                for which in names:
                    self._run(which)
        torch.cuda.current_stream().wait_stream(side)
        graphs = {}
        ops.CAPTURE_OK[0] = True          # (ops._stream() refuses captures it does not know: the autograd front end's)
        try:
            for which in names:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    s = torch.cuda.current_stream().cuda_stream
                    for plan in self._plans[which]:
                        plan.run(s)
                graphs[which] = g
        finally:
            ops.CAPTURE_OK[0] = False
        return graphs

    def _check(self, t: torch.Tensor, what: str, tail) -> None:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.VaePlayHipError(f"FusedVAEInference: {what} must be a tensor on the HIP device (no CPU path exists)")
        if t.dtype != torch.float32:
            raise _lib.VaePlayHipError(f"FusedVAEInference: {what} must be fp32, got {t.dtype}")
        if t.dim() != len(tail) + 1 or tuple(t.shape[1:]) != tuple(tail) or t.shape[0] == 0:
            raise _lib.VaePlayHipError(f"FusedVAEInference: {what} has shape {tuple(t.shape)}, this plan takes (n, {', '.join(map(str, tail))})")

    @staticmethod
    def _load(static: torch.Tensor, t: torch.Tensor) -> None:
        m = t.shape[0]
        static[:m].copy_(t, non_blocking=True)
        if m < static.shape[0]:
            static[m:].zero_()              # a short last chunk: zero rows (rows are independent in eval mode)

    def _chunks(self, n: int):
        for i0 in range(0, n, self.B):
            yield i0, min(self.B, n - i0)

    def encode(self, x: torch.Tensor):
        """(mu, logvar) of images x (n, C, S, S)"""
        self._check(x, "x", (self.C, self.S, self.S))
        n = x.shape[0]
        mu, logvar = x.new_empty((n, self.Z)), x.new_empty((n, self.Z))
        for i0, m in self._chunks(n):
            self._load(self.x_nchw, x[i0:i0 + m])
            self._run("encode")
            mu[i0:i0 + m].copy_(self.mu[:m])
            logvar[i0:i0 + m].copy_(self.logvar[:m])
        return mu, logvar

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """x_tilde (n, C, S, S) of latents z (n, Z)"""
        self._check(z, "z", (self.Z,))
        n = z.shape[0]
        out = z.new_empty((n, self.C, self.S, self.S))
        for i0, m in self._chunks(n):
            self._load(self.z, z[i0:i0 + m])
            self._run("decode")
            out[i0:i0 + m].copy_(self.x_tilde[:m])
        return out

    def reconstruct(self, x: torch.Tensor, eps: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None):
        """(x_tilde, mu, logvar): encode, z = eps * exp(logvar / 2) + mu, decode -- eval mode still SAMPLES z, as the reference's
        eval branch does; ``eps`` (n, Z) may be injected, else it is drawn from N(0, I) with ``generator``"""
        self._check(x, "x", (self.C, self.S, self.S))
        n = x.shape[0]
        if eps is None:
            eps = torch.randn((n, self.Z), dtype=torch.float32, device=x.device, generator=generator)
        self._check(eps, "eps", (self.Z,))
        if eps.shape[0] != n:
            raise _lib.VaePlayHipError(f"FusedVAEInference: eps has {eps.shape[0]} rows, x has {n}")
        out = x.new_empty((n, self.C, self.S, self.S))
        mu, logvar = x.new_empty((n, self.Z)), x.new_empty((n, self.Z))
        for i0, m in self._chunks(n):
            self._load(self.x_nchw, x[i0:i0 + m])
            self._load(self.eps, eps[i0:i0 + m])
            self._run("reconstruct")
            out[i0:i0 + m].copy_(self.x_tilde[:m])
            mu[i0:i0 + m].copy_(self.mu[:m])
            logvar[i0:i0 + m].copy_(self.logvar[:m])
        return out, mu, logvar

    # ---- scoring: per-image ELBO and importance-weighted bound -----------------------------------
    def enable_scoring(self, k_max: int = 1) -> None:
        """Allocate what ``score`` needs for up to ``k_max`` draws per image (``score`` calls this itself on first use, and again
        when it is asked for more draws).  A plan that never scores owns none of it: ``_bufs`` and the encode / decode / reconstruct
        lists of such a plan are what they were before scoring existed.  The buffers are registered like every other one
        (``PlanBuilder.buf``); asking for more draws replaces them and drops the lists (and graphs) built over the old ones."""
        k_max = int(k_max)
        if k_max < 1:
            raise ValueError("k_max must be positive")
        if self._score is not None and k_max <= self._score.k_max:
            return
        for which in [w for w in self._plans if w.startswith("score")]:
            del self._plans[which]
            self._graphs.pop(which, None)
        for name in [n for n in self._bufs if n.startswith("score.")]:
            del self._bufs[name]
        B, Z, n = self.B, self.Z, self.C * self.S * self.S
        b = PlanBuilder(self, self.dev, self.precision, side_on=False, wgrad_cus=(0, 0))
        s = SimpleNamespace(k_max=k_max, n=n)
        s.eps = b.buf("score.eps", k_max, B, Z)                 # draw-major: draw j's eps is a dense [B][Z]
        s.kl = b.buf("score.kl", B)
        # what the per-draw launches write, [draw][image] ...
        s.bce_kb, s.lr_kb = b.buf("score.bce_kb", k_max * B), b.buf("score.lr_kb", k_max * B)
        # ... and the same [image][draw], as vp_iw_bound_f32 reads it (one draw: the two orders are one)
        s.bce_bk, s.lr_bk = (b.buf("score.bce_bk", B * k_max), b.buf("score.lr_bk", B * k_max)) if k_max > 1 else (s.bce_kb, s.lr_kb)
        s.logw, s.iwae = b.buf("score.logw", B * k_max), b.buf("score.iwae", B)
        s.ws = b.ws("score.bce.ws", b.lib.vp_bce_rows_workspace_bytes(B, n))
        self._score = s

    def _score_bk(self, k: int):
        """the (bce, lr) buffers in [image][draw] order for k draws (one draw: the per-draw buffers themselves)"""
        s = self._score
        return (s.bce_kb, s.lr_kb) if k == 1 else (s.bce_bk, s.lr_bk)

    def _score_list(self, k: int) -> str:
        """name of the launch list that scores one chunk with k draws: the encode list once; per draw the reparameterisation with
        its log density ratio, the decode list and the per-image BCE; then the bound.  Built on first use."""
        which = f"score{k}"
        if which in self._plans:
            return which
        P, s, B = _ptr, self._score, self.B
        (p_enc,), (p_dec,) = self._plans["encode"], self._plans["decode"]
        plans = [p_enc]
        for j in range(k):
            lat, bce = _Plan(), _Plan()
            lat.add("vp_latent_iw_fwd_f32", P(self.mu), P(self.logvar), P(s.eps[j]), P(self.z), P(s.kl) if j == 0 else None,
                    P(s.lr_kb[j * B:]), B, self.Z)
            bce.add("vp_bce_rows_f32", P(self.x_tilde), P(self.x_nchw), B, s.n, P(s.bce_kb[j * B:]), P(s.ws), s.ws.numel() * 4)
            plans += [lat, p_dec, bce]
        fin = _Plan()
        bce_bk, lr_bk = self._score_bk(k)
        if k > 1:       # [draw][image] -> [image][draw]: the transpose kernel over one k x B "image"
            fin.add("vp_nchw_to_nhwc_f32", P(s.bce_kb), P(bce_bk), 1, k, B, 1)
            fin.add("vp_nchw_to_nhwc_f32", P(s.lr_kb), P(lr_bk), 1, k, B, 1)
        fin.add("vp_iw_bound_f32", P(bce_bk), P(lr_bk), B, k, P(s.logw), P(s.iwae))
        self._plans[which] = tuple(plans + [fin])
        if self._graphs:
            self._graphs.update(self._capture([which]))
        return which

    def score(self, x: torch.Tensor, k: int = 1, eps: Optional[torch.Tensor] = None,
              generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """How well the model explains images x (n, C, S, S), with k draws z ~ q(z | x) per image, in nats:
          bce  (n, k)  reconstruction term per image and draw: the per-pixel BCE summed over C * S * S
          kl   (n,)    analytic KL(q(z | x) || N(0, I))    (models/networks.py:270)
          logw (n, k)  log importance weight  log p(x | z) + log p(z) - log q(z | x)
          elbo (n,)    -(mean_k bce + kl)
          iwae (n,)    log-mean-exp_k logw: the k-sample importance-weighted bound (no counterpart in the reference)
        ``eps`` (n, k, Z) may be injected, else it is drawn from N(0, I) with ``generator``.  The encoder runs once per chunk, the
        decoder once per draw; ``score(x, 1, eps)`` decodes exactly what ``reconstruct(x, eps[:, 0])`` does."""
        self._check(x, "x", (self.C, self.S, self.S))
        n, k = x.shape[0], int(k)
        if k < 1:
            raise ValueError("k must be positive")
        if eps is None:
            eps = torch.randn((n, k, self.Z), dtype=torch.float32, device=x.device, generator=generator)
        self._check(eps, "eps", (k, self.Z))
        if eps.shape[0] != n:
            raise _lib.VaePlayHipError(f"FusedVAEInference: eps has {eps.shape[0]} rows, x has {n}")
        self.enable_scoring(k)
        which, s, B = self._score_list(k), self._score, self.B
        bce, logw = x.new_empty((n, k)), x.new_empty((n, k))
        kl, iwae = x.new_empty((n,)), x.new_empty((n,))
        for i0, m in self._chunks(n):
            self._load(self.x_nchw, x[i0:i0 + m])
            s.eps[:k, :m].copy_(eps[i0:i0 + m].transpose(0, 1), non_blocking=True)
            if m < B:
                s.eps[:k, m:].zero_()
            self._run(which)
            bce[i0:i0 + m].copy_(self._score_bk(k)[0][:B * k].view(B, k)[:m])
            logw[i0:i0 + m].copy_(s.logw[:B * k].view(B, k)[:m])
            kl[i0:i0 + m].copy_(s.kl[:m])
            iwae[i0:i0 + m].copy_(s.iwae[:m])
        return {"bce": bce, "kl": kl, "logw": logw, "elbo": -(bce.mean(1) + kl), "iwae": iwae}

    # ---- latent projection: the decoder's input gradient and Adam on z ----------------------------------------------------------
    _PROJECT_DEFAULTS = (0.05, 0.9, 0.999, 1e-8, 1.0)        # lr, beta1, beta2, eps, prior_weight of ``project``

    def enable_projection(self) -> None:
        """Allocate and plan what ``project`` / ``decode_grad`` need (they call this themselves on first use).  A plan that never
        projects owns none of it: ``_bufs`` and the encode / decode / reconstruct / score lists of such a plan are what they were
        before projection existed.  Everything new is registered like every other buffer (``PlanBuilder.buf / sbuf / ws``) under a
        ``project.`` prefix: the gather-family packs of the decoder blocks (the eval plan owns the scatter family only), the gradient
        ping-pong buffers and the split gradient plane, Adam's moments and its step counter, and NHWC copies of target and mask when
        the image has more than one channel.

        "f16" plans refuse: their activations are fp16 hi planes alone, which flush small positive values to zero, so the ReLU mask
        is not recoverable from a block's output, and there are no one-product input-gradient kernels."""
        if self._proj is not None:
            return
        if self.precision == "f16":
            raise NotImplementedError("FusedVAEInference: projection needs a 'bf16x3' or 'f32' plan (an 'f16' plan keeps fp16 hi planes "
                                      "only: the ReLU masks are not recoverable from them, and no one-product gradient kernels exist)")
        B, S, C, Z, P = self.B, self.S, self.C, self.Z, _ptr
        trunk, ps = self._trunk, self._dec_pass
        n = C * S * S
        b = PlanBuilder(self, self.dev, self.precision, side_on=False, wgrad_cus=(0, 0))
        q = SimpleNamespace(n=n, hyper=None)
        # the input-gradient packs
        p0s = []
        for i, blk in enumerate(ps.blocks):
            alloc, sfx = (b.sbuf, "s") if blk.is16 else (b.buf, "")
            p0s.append(alloc(f"project.dec{i}.p0{sfx}", blk.Cin * 25 * blk.Cout))
            b.pack(blk.blk.conv.weight, p0s[-1], None, blk.Cin, blk.Cout, blk.is16)
        fin, fin_p1 = trunk.fin, None
        if not fin.edge:
            fin_p1 = b.buf("project.fin.p1", fin.Cf * 25 * C)
            b.pack(fin.conv.weight, None, fin_p1, C, fin.Cf, False)
        # target, mask, objective
        q.mask = b.buf("project.mask", B, C, S, S)
        load = _Plan()
        if C > 1:
            q.x_nhwc, q.mask_nhwc = b.buf("project.x_nhwc", B * n), b.buf("project.mask_nhwc", B * n)
            load.add("vp_nchw_to_nhwc_f32", P(self.x_nchw), P(q.x_nhwc), B, C, S, S)
            load.add("vp_nchw_to_nhwc_f32", P(q.mask), P(q.mask_nhwc), B, C, S, S)
        else:
            q.x_nhwc, q.mask_nhwc = self.x_nchw, q.mask
        q.bce, q.prior = b.buf("project.bce", B), b.buf("project.prior", B)
        dlogit = b.buf("project.dlogit", B * n)
        ws = b.ws("project.bce.ws", b.lib.vp_bce_masked_rows_bwd_workspace_bytes(B, n))
        bce = _Plan()
        bce.add("vp_bce_masked_rows_bwd_f32", P(self._xt_nhwc), P(q.x_nhwc), P(q.mask_nhwc), B, n, P(q.bce), P(dlogit), P(ws),
                ws.numel() * 4)
        # the walk back to z
        n_g = max([B * trunk.F1] + [blk.R * blk.Cout for blk in ps.blocks])
        cur, other = b.buf("project.gA", n_g), b.buf("project.gB", n_g)
        n_s = max([0] + [blk.R * blk.Cout for blk in ps.blocks if blk.is16])
        g_s = b.sbuf("project.gS", n_s) if n_s else None
        q.dz = b.buf("project.dz", B, Z)
        walk = _Plan()
        trunk.bwd_eval(walk, b, ps, dlogit, cur, other, g_s, p0s, q.dz, fin_p1)
        # Adam's state; the step counter is an int32 in device memory
        q.m, q.v = b.buf("project.m", B, Z), b.buf("project.v", B, Z)
        q.step = b.buf("project.step", 1).view(torch.int32)
        q.prep = _Plan()
        b.finish(q.prep, prefix="project.")
        q.p_bce, q.walk = bce, walk
        self._proj = q
        if load.calls:
            self._plans["project.load"] = (load,)
        self._project_lists(*self._PROJECT_DEFAULTS)
        if self.dev.type == "cuda":
            q.prep.run(torch.cuda.current_stream().cuda_stream)

    def _project_lists(self, lr: float, beta1: float, beta2: float, eps: float, prior_weight: float) -> None:
        """The launch lists that end in a launch with these hyper-parameters in its arguments, rebuilt (and captured again) when they
        change:
          "project"       one iteration: the decode list, the masked per-image BCE with dlogit, the input-gradient walk to dz, the latent
                          update (which also leaves the prior term of the z it read)
          "project.grad"  the same without the update (``decode_grad``)
          "project.loss"  the decode list, the BCE and the prior term: the loss at a z"""
        q, P = self._proj, _ptr
        hyper = (float(lr), float(beta1), float(beta2), float(eps), float(prior_weight))
        if q.hyper == hyper:
            return
        (p_dec,) = self._plans["decode"]
        adam, prior = _Plan(), _Plan()
        adam.add("vp_latent_adam_f32", P(self.z), P(q.dz), P(q.m), P(q.v), P(q.step), self.B, self.Z, *hyper, P(q.prior))
        prior.add("vp_latent_adam_f32", P(self.z), None, None, None, None, self.B, self.Z, 0.0, 0.0, 0.0, 0.0, hyper[4], P(q.prior))
        self._plans["project"] = (p_dec, q.p_bce, q.walk, adam)
        self._plans["project.grad"] = (p_dec, q.p_bce, q.walk, prior)
        self._plans["project.loss"] = (p_dec, q.p_bce, prior)
        q.hyper = hyper
        if self._graphs:
            self._graphs.update(self._capture([w for w in self._plans if w.startswith("project")]))

    def _project_load(self, x: torch.Tensor, mask: Optional[torch.Tensor], i0: int, m: int) -> None:
        """target and mask of one chunk into the plan's buffers; the zero rows of a short chunk get a zero mask (no loss, no gradient)"""
        q = self._proj
        self._load(self.x_nchw, x[i0:i0 + m])
        if mask is None:
            q.mask[:m].fill_(1.0)
            q.mask[m:].zero_()
        else:
            self._load(q.mask, mask[i0:i0 + m])
        if "project.load" in self._plans:
            self._run("project.load")

    def _project_args(self, x, mask, prior_weight):
        self._check(x, "x", (self.C, self.S, self.S))
        if mask is not None:
            self._check(mask, "mask", (self.C, self.S, self.S))
            if mask.shape[0] != x.shape[0]:
                raise _lib.VaePlayHipError(f"FusedVAEInference: mask has {mask.shape[0]} rows, x has {x.shape[0]}")
        if not prior_weight >= 0.0:
            raise ValueError("prior_weight must be non-negative")

    def decode_grad(self, z: torch.Tensor, x: torch.Tensor, mask: Optional[torch.Tensor] = None,
                    prior_weight: float = 0.0) -> Dict[str, torch.Tensor]:
        """The projection objective at latents z (n, Z) for images x (n, C, S, S) and its gradient; nothing is updated:
          x_tilde (n, C, S, S)  decode(z)
          bce     (n,)          sum over the image of mask * per-pixel BCE(x_tilde, x)   (``mask``: fp32, the shape of x, weights in
                                [0, 1]; None: all ones)
          loss    (n,)          bce + prior_weight / 2 |z|^2
          dz      (n, Z)        d loss / d z through the frozen decoder in eval mode
        No counterpart in the reference (new functionality).  Needs a "bf16x3" or "f32" plan."""
        self._check(z, "z", (self.Z,))
        self._project_args(x, mask, prior_weight)
        if x.shape[0] != z.shape[0]:
            raise _lib.VaePlayHipError(f"FusedVAEInference: x has {x.shape[0]} rows, z has {z.shape[0]}")
        self.enable_projection()
        lr, b1, b2, eps, _ = self._proj.hyper
        self._project_lists(lr, b1, b2, eps, prior_weight)
        q, n = self._proj, z.shape[0]
        out = {"x_tilde": x.new_empty((n, self.C, self.S, self.S)), "bce": x.new_empty((n,)), "loss": x.new_empty((n,)),
               "dz": z.new_empty((n, self.Z))}
        for i0, m in self._chunks(n):
            self._load(self.z, z[i0:i0 + m])
            self._project_load(x, mask, i0, m)
            self._run("project.grad")
            out["x_tilde"][i0:i0 + m].copy_(self.x_tilde[:m])
            out["bce"][i0:i0 + m].copy_(q.bce[:m])
            out["loss"][i0:i0 + m].copy_((q.bce + q.prior)[:m])
            out["dz"][i0:i0 + m].copy_(q.dz[:m] if prior_weight == 0.0 else q.dz[:m] + prior_weight * self.z[:m])
        return out

    def project(self, x: torch.Tensor, steps: int = 100, lr: float = 0.05, mask: Optional[torch.Tensor] = None, z0="encode",
                prior_weight: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8, history: bool = False) -> Dict[str, torch.Tensor]:
        """Search the latent space for images x (n, C, S, S): ``steps`` iterations of Adam (torch.optim.Adam's update, no amsgrad, no
        weight decay) on   loss(z) = sum over the image of mask * BCE(decode(z), x) + prior_weight / 2 |z|^2   per image, from
        ``z0``: "encode" (the encoder mean of x), "zeros", or an (n, Z) tensor.  ``mask``: fp32, the shape of x, weights in [0, 1]
        (inpainting, occlusion-robust scoring); None: all ones.  Returns
          z (n, Z), x_tilde (n, C, S, S), loss (n,)   at the final z
          history (steps, n)   with ``history=True``: the loss at the z each iteration started from
        One iteration is ONE launch list (the decode list, the masked BCE, the input-gradient walk, the latent update) replayed
        ``steps`` times -- as a hipGraph after ``capture()``, with the same bits: Adam's step count lives in device memory.  Rows are
        independent (eval-mode decoder, elementwise Adam).  Every call starts from step 1 with zero moments.
        No counterpart in the reference (new functionality).  Needs a "bf16x3" or "f32" plan."""
        self._project_args(x, mask, prior_weight)
        n, steps = x.shape[0], int(steps)
        if steps < 0:
            raise ValueError("steps must not be negative")
        if isinstance(z0, torch.Tensor):
            self._check(z0, "z0", (self.Z,))
            if z0.shape[0] != n:
                raise _lib.VaePlayHipError(f"FusedVAEInference: z0 has {z0.shape[0]} rows, x has {n}")
        elif z0 not in ("encode", "zeros"):
            raise ValueError("z0 must be 'encode', 'zeros' or an (n, Z) tensor")
        self.enable_projection()
        self._project_lists(lr, betas[0], betas[1], eps, prior_weight)
        q = self._proj
        out = {"z": x.new_empty((n, self.Z)), "x_tilde": x.new_empty((n, self.C, self.S, self.S)), "loss": x.new_empty((n,))}
        if history:
            out["history"] = x.new_empty((steps, n))
        for i0, m in self._chunks(n):
            self._project_load(x, mask, i0, m)
            if isinstance(z0, torch.Tensor):
                self._load(self.z, z0[i0:i0 + m])
            elif z0 == "encode":
                self._run("encode")
                self.z.copy_(self.mu)
            else:
                self.z.zero_()
            q.m.zero_()
            q.v.zero_()
            q.step.zero_()
            for it in range(steps):
                self._run("project")
                if history:
                    out["history"][it, i0:i0 + m].copy_((q.bce + q.prior)[:m])
            self._run("project.loss")
            out["z"][i0:i0 + m].copy_(self.z[:m])
            out["x_tilde"][i0:i0 + m].copy_(self.x_tilde[:m])
            out["loss"][i0:i0 + m].copy_((q.bce + q.prior)[:m])
        return out

    def sample(self, n: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """x_p (n, C, S, S): decode z_p ~ N(0, I) (the reference's ``x is None`` branch)"""
        if n <= 0:
            raise ValueError("n must be positive")
        return self.decode(torch.randn((n, self.Z), dtype=torch.float32, device=self.dev, generator=generator))
