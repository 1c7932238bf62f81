"""Fused VAE-GAN inference: what ``infer.FusedVAEInference`` does for the encoder / decoder halves, for the whole ``networks.VaeGan``
-- the circle parameters of ``param_encoder`` next to the reconstruction (the eval branch of VaeGan.forward, models/networks.py:248-258),
the discriminator's real / fake probability and its features (modes "GAN" and "REC", :174-198, in eval mode), and per image the terms
of VaeGan.loss (:265-281) that compare an image with its reconstruction: the learned similarity the model is trained on.

Two things are folded when the plan is (re)built, not per call:
  * every eval-mode BatchNorm, as in the parent;
  * ``DirectDecoder`` (:118-148): eight bias-ed Linear layers with NO activation are one affine map params = W_eff z + b_eff
    (3 x Z).  It is folded from the output side -- [r_fc.1 r_fc.0 ; xy_fc.1 xy_fc.0] (3 x 64), times head.3 .. head.0 in turn, the bias
    carried along as W_out b + b_out -- so that every intermediate product has three rows, by six launches of ``vp_lin_fold_f32``.
    ``params`` is then ONE dense launch where the module path runs eight.

The discriminator runs over 2B rows, two halves of B (sections.DiscriminatorEval): in ``similarity`` half a reads the plan's image
buffer and half b the decode list's output where it lies -- nothing is concatenated or copied.  DESIGN.md 14.4.
"""
from __future__ import annotations

from ctypes import c_void_p
from types import SimpleNamespace
from typing import Dict, Optional

import torch

from . import _lib, sections
from .infer import FusedVAEInference
from .plan import PlanBuilder, _Plan, _ptr


class FusedVAEGANInference(FusedVAEInference):
    """``FusedVAEInference`` over ``net.encoder`` / ``net.decoder`` of a ``networks.VaeGan`` (one image channel, the image size from
    ``net.iter_level``) -- encode / decode / reconstruct / sample / score / project / capture are the parent's, launch for launch --
    plus ``params``, ``forward``, ``discriminate`` and ``similarity``.

    What the new methods need is built by ``enable_gan()`` (they call it on first use); a plan that never uses them owns no buffer
    and no list beyond the parent's.  The new buffers carry a ``gan.`` prefix.  ``params`` and ``forward`` work in every precision
    the parent takes; ``discriminate`` and ``similarity`` need a "bf16x3" plan (the discriminator's stem and blocks are the
    split-bf16 kernels, as in the fused training step).

    The parent's contract holds: the plan SNAPSHOTS the model -- the folded DirectDecoder and the discriminator's packs and folded
    BatchNorms included; after the module's parameters or buffers change, always call ``refresh()``.  Nothing here writes to the module."""

    def __init__(self, net, batch_size: int, precision: str = "bf16x3", _plan_only: bool = False):
        disc = net.discriminator
        if disc.recon_levl != len(disc.conv) - 1:
            raise NotImplementedError("the fused plan taps the discriminator's last block (VaeGan's own construction)")
        self.net = net
        self._gan: Optional[SimpleNamespace] = None         # the VAE-GAN buffers and lists: none until enable_gan()
        self._init(net.encoder, net.decoder, batch_size, 8 * 2 ** int(net.iter_level), 1, precision, _plan_only)

    # ---- plan construction ------------------------------------------------------------------
    def enable_gan(self) -> None:
        """Allocate and plan what ``params`` / ``forward`` / ``discriminate`` / ``similarity`` need.  Lists (each a tuple of ``_Plan``s,
        single-stream, allocation-free, captured like the parent's):
          "gan.params"        one dense launch over the folded map
          "gan.forward"       the parent's reconstruct list (the same ``_Plan`` objects), then gan.params
          "gan.discriminate"  stem (both halves from the staging buffer ``gan.x``), blocks, tap with the features, head
          "gan.similarity"    encode, the reparameterisation with the KL term, decode, gan.params, stem (half a: the image buffer,
                              half b: the decode list's output), blocks, tap with the feature distance, head, the pixel term
        and the prep list (run by ``refresh()``): the discriminator's weight pack, one fold per discriminator BatchNorm, the six
        folds of DirectDecoder.  The discriminator lists exist on "bf16x3" plans only."""
        if self._gan is not None:
            return
        B, S, Z, P = self.B, self.S, self.Z, _ptr
        b = PlanBuilder(self, self.dev, self.precision, side_on=False, wgrad_cus=(0, 0))
        g = SimpleNamespace(prep=_Plan(), disc=None)
        prep = g.prep

        # ---- DirectDecoder as one affine map ----
        pe = self.net.param_encoder
        heads = list(pe.head)
        tails = (pe.r_fc, pe.xy_fc)
        n_out = sum(t[1].weight.shape[0] for t in tails)
        width = max([tails[0][0].weight.shape[1]] + [lin.weight.shape[1] for lin in heads[1:]])
        g.w_eff, g.b_eff = b.buf("gan.w_eff", n_out, Z), b.buf("gan.b_eff", n_out)
        fold_w = [b.buf(f"gan.fold.w{j}", n_out * width) for j in range(2)]
        fold_b = [b.buf(f"gan.fold.b{j}", n_out) for j in range(2)]

        def at(t: torch.Tensor, off: int):
            return c_void_p(t.data_ptr() + 4 * off)
        row, K = 0, tails[0][0].weight.shape[1]
        for fc in tails:                       # [r_fc.1 r_fc.0 ; xy_fc.1 xy_fc.0], rows in the order of the reference's cat([r, xy])
            M, N = fc[1].weight.shape
            prep.add("vp_lin_fold_f32", P(fc[1].weight), P(fc[1].bias), P(fc[0].weight), P(fc[0].bias), M, N, K, at(fold_w[0], row * K),
                     at(fold_b[0], row), tag="gan.fold")
            row += M
        cur = 0
        for j in range(len(heads) - 1, -1, -1):          # ... times head.3 .. head.0
            N, K = heads[j].weight.shape
            w_new, b_new = (g.w_eff, g.b_eff) if j == 0 else (fold_w[1 - cur], fold_b[1 - cur])
            prep.add("vp_lin_fold_f32", P(fold_w[cur]), P(fold_b[cur]), P(heads[j].weight), P(heads[j].bias), n_out, N, K, P(w_new),
                     P(b_new), tag="gan.fold")
            cur = 1 - cur
        g.params = b.buf("gan.params", B, n_out)
        g.n_out = n_out
        p_par = _Plan()
        b.lin_fwd(p_par, self.z, g.w_eff, g.b_eff, g.params, B, n_out, Z)
        self._plans["gan.params"] = (p_par,)
        self._plans["gan.forward"] = self._plans["reconstruct"] + (p_par,)

        # ---- the discriminator over (x | x_tilde) ----
        if self.precision == "bf16x3":
            d = g.disc = sections.DiscriminatorEval(b, self.net.discriminator, B, S, prep)
            g.x = b.buf("gan.x", 2 * B, 1, S, S)
            g.features = b.buf("gan.features", 2 * B, d.nf)
            g.kl, g.mse, g.nle = b.buf("gan.kl", B), b.buf("gan.mse", B), b.buf("gan.nle", B)
            stem_x, tap_x, stem_s, tap_s, lat, nle = (_Plan() for _ in range(6))
            d.stem(stem_x, g.x[:B], g.x[B:])
            d.tap(tap_x, g.features, 0, None)
            self._plans["gan.discriminate"] = (stem_x, d.body, tap_x, d.head)
            (p_enc,), (p_dec,) = self._plans["encode"], self._plans["decode"]
            # (the parent's reparameterisation launch, which writes the same z, with the KL term's pointer given)
            lat.add("vp_latent_fwd_f32", P(self.mu), P(self.logvar), P(self.eps), P(self.z), P(g.kl), B, Z)
            d.stem(stem_s, self.x_nchw, self._xt_nhwc)
            d.tap(tap_s, None, B, g.mse)
            nle.add("vp_half_sqdiff_rowsum_f32", P(self.x_nchw), P(self._xt_nhwc), P(g.nle), B, S * S)
            self._plans["gan.similarity"] = (p_enc, lat, p_dec, p_par, stem_s, d.body, tap_s, d.head, nle)
            b.finish(prep, prefix="gan.")       # the discriminator's batched weight pack at the head of prep; the dense workspace
        else:                                   # no 5x5 layer, nothing to pack: the dense workspace alone
            b.dense_workspace(prefix="gan.")
        self._gan = g
        if self.dev.type == "cuda":
            prep.run(torch.cuda.current_stream().cuda_stream)
            if self._graphs:
                self._graphs.update(self._capture([w for w in self._plans if w.startswith("gan.")]))

    def _need_disc(self, what: str):
        self.enable_gan()
        if self._gan.disc is None:
            raise NotImplementedError(f"FusedVAEGANInference: {what} needs a 'bf16x3' plan (the discriminator's stem and blocks are the "
                                      f"split-bf16 kernels; no exact-f32 or one-product fp16 stem exists), this plan is '{self.precision}'")
        return self._gan, self._gan.disc

    def refresh(self) -> None:
        """The parent's ``refresh()``, and once ``enable_gan()`` has run the VAE-GAN prep list too: the discriminator's weight pack
        and BatchNorm folds and the fold of DirectDecoder.  Graphs captured before are captured again."""
        if self._gan is not None:
            self._gan.prep.run(torch.cuda.current_stream().cuda_stream)
        super().refresh()

    # ---- execution ---------------------------------------------------------------------------
    def params(self, z: torch.Tensor) -> torch.Tensor:
        """(n, 3): ``param_encoder(z)`` of latents z (n, Z), cat([r, xy], -1) as the reference orders it"""
        self._check(z, "z", (self.Z,))
        self.enable_gan()
        g, n = self._gan, z.shape[0]
        out = z.new_empty((n, g.n_out))
        for i0, m in self._chunks(n):
            self._load(self.z, z[i0:i0 + m])
            self._run("gan.params")
            out[i0:i0 + m].copy_(g.params[:m])
        return out

    def _x_eps(self, x, eps, generator):
        self._check(x, "x", (self.C, self.S, self.S))
        n = x.shape[0]
        if eps is None:
            eps = torch.randn((n, self.Z), dtype=torch.float32, device=x.device, generator=generator)
        self._check(eps, "eps", (self.Z,))
        if eps.shape[0] != n:
            raise _lib.VaePlayHipError(f"FusedVAEInference: eps has {eps.shape[0]} rows, x has {n}")
        return eps

    def forward(self, x: torch.Tensor, eps: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None):
        """(x_tilde, params): the reference's eval branch with ``x`` given -- encode, z = eps * exp(logvar / 2) + mu, decode, and the
        circle parameters of that z.  It decodes exactly what ``reconstruct(x, eps)`` decodes."""
        eps = self._x_eps(x, eps, generator)
        self.enable_gan()
        g, n = self._gan, x.shape[0]
        out, par = x.new_empty((n, self.C, self.S, self.S)), x.new_empty((n, g.n_out))
        for i0, m in self._chunks(n):
            self._load(self.x_nchw, x[i0:i0 + m])
            self._load(self.eps, eps[i0:i0 + m])
            self._run("gan.forward")
            out[i0:i0 + m].copy_(self.x_tilde[:m])
            par[i0:i0 + m].copy_(g.params[:m])
        return out, par

    def discriminate(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The discriminator on images x (n, 1, S, S), in eval mode, from ONE pass over its stack:
          p        (n,)           sigmoid score (mode "GAN"): the probability that the image is real
          logit    (n,)           the same before the sigmoid
          features (n, 64 * Cd)   mode "REC": the pre-BatchNorm output of conv[recon_level], flattened in NCHW order
        The stack runs over chunks of 2 * batch_size rows (the two halves ``similarity`` fills with x and x_tilde)."""
        g, d = self._need_disc("discriminate")
        self._check(x, "x", (self.C, self.S, self.S))
        n, n2 = x.shape[0], 2 * self.B
        out = {"p": x.new_empty((n,)), "logit": x.new_empty((n,)), "features": x.new_empty((n, d.nf))}
        for i0 in range(0, n, n2):
            m = min(n2, n - i0)
            self._load(g.x, x[i0:i0 + m])
            self._run("gan.discriminate")
            out["p"][i0:i0 + m].copy_(d.p[:m])
            out["logit"][i0:i0 + m].copy_(d.logit[:m])
            out["features"][i0:i0 + m].copy_(g.features[:m])
        return out

    def similarity(self, x: torch.Tensor, eps: Optional[torch.Tensor] = None,
                   generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """How the model sees images x (n, 1, S, S) next to their reconstructions, per image, as ONE launch list:
          x_tilde (n, 1, S, S), mu, logvar (n, Z), params (n, 3)    as ``forward`` / ``reconstruct``
          kl                 (n,)  KL(q(z | x) || N(0, I))                                   (models/networks.py:270)
          nle                (n,)  1/2 sum over the pixels of (x - x_tilde)^2                (:267, summed over the image)
          mse                (n,)  1/2 sum over the features of (f(x) - f(x_tilde))^2        (:273: the learned similarity)
          p_x, p_x_tilde     (n,)  the discriminator's score of the image and of its reconstruction
          bce_dis_original   (n,)  -log(p_x + 1e-3)                                          (:274)
          bce_dis_predicted  (n,)  -log(1 - p_x_tilde + 1e-3)                                (:275)
        ``eps`` (n, Z) may be injected, else it is drawn from N(0, I) with ``generator``."""
        g, d = self._need_disc("similarity")
        eps = self._x_eps(x, eps, generator)
        n, B = x.shape[0], self.B
        vec = ("kl", "nle", "mse", "p_x", "p_x_tilde", "bce_dis_original", "bce_dis_predicted")
        out = {"x_tilde": x.new_empty((n, self.C, self.S, self.S)), "mu": x.new_empty((n, self.Z)), "logvar": x.new_empty((n, self.Z)),
               "params": x.new_empty((n, g.n_out)), **{k: x.new_empty((n,)) for k in vec}}
        for i0, m in self._chunks(n):
            self._load(self.x_nchw, x[i0:i0 + m])
            self._load(self.eps, eps[i0:i0 + m])
            self._run("gan.similarity")
            src = {"x_tilde": self.x_tilde, "mu": self.mu, "logvar": self.logvar, "params": g.params, "kl": g.kl, "nle": g.nle,
                   "mse": g.mse, "p_x": d.p, "p_x_tilde": d.p[B:], "bce_dis_original": d.nl_real, "bce_dis_predicted": d.nl_fake[B:]}
            for k, t in src.items():
                out[k][i0:i0 + m].copy_(t[:m])
        return out
