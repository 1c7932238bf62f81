"""Fused inference for the Style-GAN row (``network_Style_GAN.Generator`` / ``StyleEncoder`` / ``Discriminator``): what the reference's
``train_Style_GAN.py:148-153,279-280`` does with the nets under ``torch.no_grad()`` -- encode a style image, generate from a content
image, a style code and a class, score the result -- as fixed, pre-planned, hipGraph-replayable lists of HIP launches.

  * the three activation-free ``Generator.mlp`` layers are ONE dense launch over a map folded per ``refresh()``: W3 W2 W1 and
    W3 (W2 b1 + b2) + b3 (at 256 / 512 it reads 134 MB where the three layers read 1.5 GB);
  * ``torch.cat`` never runs: the generator's (image | style plane) and the discriminator's (x | x_content) inputs are one
    ``vp_cat2_nhwc_f32`` launch from either memory layout, and in ``StyleUp`` the transposed convolution's InstanceNorm and the skip
    block's InstanceNorm each write their channel slice of ``cat_convs.0``'s input;
  * a ``myConv2d`` is, with per-image labels, the stacked convolution + ``vp_pair_blend_fwd_f32`` of the module (the stacked weight
    built per ``refresh()``, not per call), and with ONE class for the whole batch (``labels`` a Python int 0 | 1) that branch's
    convolution alone: half the work, no blend pass;
  * the two SCSEBlocks that end ``StyleUp.cat_convs`` are one ``vp_scse2_fwd_f32`` (two passes over the tensor instead of six), which
    also writes the bf16 planes the next transposed convolution reads;
  * ``final.3`` + tanh is one launch that writes the NCHW result; ``fc_mu`` / ``fc_logvar`` are one dense launch over stacked weights;
    the discriminator's output stage is ``vp_twin_head_fwd_f32``.
Each of the new kernels and the fold is used where ``vp_scse2_preferred`` / ``vp_sg_out_tanh_preferred`` / ``_mlp_fold_preferred`` say
so, else the launches it replaces (DESIGN.md 17.1 has the measurements).

``precision`` selects the arithmetic of the layers on the existing convolution entries only -- "f32" (exact fp32 products) or "bf16x3"
(split-bf16 operands; layers whose input channel count is no multiple of 8 stay exact fp32); the new kernels and the dense layers are
always exact fp32.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional

import torch

from . import _lib, network_Style_GAN, ops
from .blocks import _CONV_LRELU
from .infer import FusedVAEInference
from .infer_font import _IN_EPS, FusedFontInference, _slice
from .plan import PlanBuilder, _Plan, _ptr, plan_device

_MODES = ("blend", "c0", "c1")      # per-image labels | every image of class 0 | of class 1


def _mlp_fold_preferred(image_size: int, z_dim: int) -> bool:
    """host-only: fold Generator.mlp into one S^2 x z map (one dense launch) instead of its three layers"""
    return True


class FusedStyleGanInference:
    """``generate`` / ``encode_style`` / ``stylize`` / ``discriminate`` of a ``network_Style_GAN.Generator`` and, when given, a
    ``StyleEncoder`` and a ``Discriminator`` of the same ``image_size`` S (a power of two >= 32), on (n, 3, S, S) fp32 images,
    contiguous or channels_last.

    The plan SNAPSHOTS the modules when it is built: convolution weights are stacked and packed, ``mlp`` is folded and the two
    ``fc`` heads are stacked into plan-owned buffers once, not per call.  After a module's parameters change call ``refresh()``;
    until then the plan keeps computing with what it was built with.  Nothing here writes to the modules and their ``training``
    flags are left as found.  Inputs of any number of images run in chunks of ``batch_size``; a short last chunk is padded with zero
    images."""

    _run, _capture, _chunks = FusedVAEInference._run, FusedVAEInference._capture, FusedVAEInference._chunks
    _load = staticmethod(FusedVAEInference._load)
    # the emitters of the font plan: the k x k convolution entry, convolution + InstanceNorm, the bf16 planes of a buffer, Linear
    _gather, _in_conv, _split_of, _dense = (FusedFontInference._gather, FusedFontInference._in_conv, FusedFontInference._split_of,
                                            FusedFontInference._dense)

    def __init__(self, generator, style_encoder=None, discriminator=None, batch_size: int = 1, precision: str = "bf16x3",
                 _plan_only: bool = False):
        N = network_Style_GAN
        if precision not in ("f32", "bf16x3"):
            raise ValueError("precision must be 'f32' or 'bf16x3'")
        if not isinstance(generator, N.Generator):
            raise ValueError("FusedStyleGanInference takes a network_Style_GAN.Generator")
        if style_encoder is not None and not isinstance(style_encoder, N.StyleEncoder):
            raise ValueError("style_encoder must be a network_Style_GAN.StyleEncoder or None")
        if discriminator is not None and not isinstance(discriminator, N.Discriminator):
            raise ValueError("discriminator must be a network_Style_GAN.Discriminator or None")
        if not isinstance(batch_size, int) or batch_size <= 0:
            raise ValueError("batch_size must be positive")
        S = int(generator.image_size)
        if S < 32 or S & (S - 1):
            raise ValueError(f"image_size must be a power of two >= 32 (at 16 down4 is one pixel, which InstanceNorm cannot take), got {S}")
        if style_encoder is not None:
            if 2 ** (len(style_encoder.convs) - 1) != S:
                raise ValueError(f"style_encoder was built for image_size {2 ** (len(style_encoder.convs) - 1)}, the generator for {S}")
            if style_encoder.fc_mu.fc[0].weight.shape[0] != generator.z_dim:
                raise ValueError("style_encoder and generator differ in z_dim")
        if discriminator is not None and 2 ** (len(discriminator.convs) + 1) != S:
            raise ValueError(f"discriminator was built for image_size {2 ** (len(discriminator.convs) + 1)}, the generator for {S}")
        self.generator, self.style_encoder, self.discriminator = generator, style_encoder, discriminator
        self.precision, self.S, self.B, self.Z = precision, S, int(batch_size), int(generator.z_dim)
        self.K = discriminator.num_of_classes if discriminator is not None else 0
        self.dev = plan_device(generator, "FusedStyleGanInference", _plan_only)
        self._bufs: Dict[str, torch.Tensor] = {}
        self._graphs: Dict[str, "torch.cuda.CUDAGraph"] = {}
        self._planes: Dict[int, torch.Tensor] = {}
        self._stacks = []               # (plan-owned buffer, the module tensors stacked into it along dim 0): refresh() copies
        self._build()
        if not _plan_only:
            self.refresh()

    # ---- plan construction: one emitter per kind of block ---------------------------------------------------------------------
    def _stacked(self, name, tensors):
        t = self._b.buf(name, sum(x.shape[0] for x in tensors), *tensors[0].shape[1:])
        self._stacks.append((t, tuple(tensors)))
        return t

    def _scatter(self, plan, prep, tag, ct, src, Hs, Ws, out):
        """ConvTranspose2d(in, out, 4, 2, 1) with its bias in the plan's arithmetic: the existing scatter entry"""
        B, P, b = self.B, _ptr, self._b
        cs, cb = ct.weight.shape[0], ct.weight.shape[1]
        geom = (B, Hs, Ws, 2 * Hs, 2 * Ws, cs, cb, 4, 2)
        flops = 2.0 * B * Hs * Ws * cs * cb * 16
        if self.precision == "bf16x3" and cs % 8 == 0 and cb % 8 == 0:
            p1 = b.sbuf(f"{tag}.p1s", cs * cb * 16)
            prep.add("vp_pack_w_split", P(ct.weight), None, P(p1), cs, cb, 4, tag=f"{tag}.pack")
            xs = self._split_of(plan, tag, src)
            plan.add("vp_conv_scatter_bias_bf16x3", P(xs), P(p1), P(ct.bias), P(out), *geom, flops=flops, tag=f"{tag}.fwd")
        else:
            p1 = b.buf(f"{tag}.p1", cb, 16, cs)
            prep.add("vp_pack_w_f32", P(ct.weight), None, P(p1), cs, cb, 4, tag=f"{tag}.pack")
            plan.add("vp_conv_scatter_bias_f32", P(src), P(p1), P(ct.bias), P(out), *geom, flops=flops, tag=f"{tag}.fwd")

    def _bias_conv(self, plan, prep, tag, block, src, H, W):
        """blocks.Conv2d(bn=None): ONE gather with bias and ReLU (or no activation) in the epilogue; LeakyReLU is one pass more"""
        conv = block.conv[0]
        act = block.conv[1].act if len(block.conv) > 1 else None
        cout, cin, ks, stride = conv.weight.shape[0], conv.weight.shape[1], conv.kernel_size, conv.stride
        pad = (ks - 1) // 2
        Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        y = self._b.buf(f"{tag}.y", self.B, Ho, Wo, cout)
        if act not in (None, "relu", "lrelu"):
            raise ValueError(f"{tag}: activation {act} is not one the fused bias blocks take")
        self._gather(plan, prep, tag, conv.weight, conv.bias, src, H, W, cout, cin, ks, stride,
                     ops.ACT_RELU if act == "relu" else ops.ACT_NONE, y)
        if act == "lrelu":
            plan.add("vp_act_fwd_f32", _ptr(y), _ptr(y), y.numel(), ops.ACT_LRELU, float(block.conv[1].slope), tag=f"{tag}.act")
        return y, Ho, Wo

    def _my_conv(self, plan, prep, tag, m, mode, src, H, W):
        """myConv2d: "blend" = the stacked convolution + vp_pair_blend_fwd_f32, as the module; "c0" / "c1" = that branch alone"""
        B, P, b = self.B, _ptr, self._b
        norm = m.bn == "instance"
        if mode != "blend":
            branch = m.conv_1 if mode == "c0" else m.conv_2
            return self._in_conv(plan, prep, tag, branch, src, H, W) if norm else self._bias_conv(plan, prep, tag, branch, src, H, W)
        p1, p2 = m.conv_1.conv[0], m.conv_2.conv[0]
        C, cin, ks = p1.weight.shape[0], p1.weight.shape[1], p1.kernel_size
        wst = self._stacked(f"{tag}.wst", (p1.weight, p2.weight))
        bst = None if p1.bias is None else self._stacked(f"{tag}.bst", (p1.bias, p2.bias))
        pad = (ks - 1) // 2
        Ho, Wo = (H + 2 * pad - ks) // m.stride + 1, (W + 2 * pad - ks) // m.stride + 1
        u, y = b.buf(f"{tag}.u", B, Ho, Wo, 2 * C), b.buf(f"{tag}.y", B, Ho, Wo, C)
        self._gather(plan, prep, tag, wst, bst, src, H, W, 2 * C, cin, ks, m.stride, ops.ACT_NONE, u)
        ys = mean = rstd = ws = None
        if self.precision == "bf16x3" and C % 8 == 0:
            ys = b.sbuf(f"{tag}.ys", y.numel())
            self._planes[y.data_ptr()] = ys
        if norm:
            mean, rstd = b.buf(f"{tag}.mean", B, 2 * C), b.buf(f"{tag}.rstd", B, 2 * C)
            ws = b.ws(f"{tag}.pbws", _lib.load().vp_pair_blend_workspace_bytes(B, Ho * Wo, C))
        plan.add("vp_pair_blend_fwd_f32", P(u), P(self.label), P(y), P(ys), P(mean), P(rstd), B, Ho * Wo, C, int(norm), _IN_EPS,
                 ops.ACT_CODES[m.act], _CONV_LRELU, P(ws), ws.numel() * 4 if ws is not None else 0, tag=f"{tag}.blend")
        return y, Ho, Wo

    def _scse_pair(self, plan, tag, blk_a, blk_b, x, H, W):
        """relu(SCSE_b(SCSE_a(x))): ONE vp_scse2_fwd_f32 where vp_scse2_preferred says so, else two vp_scse_fwd_f32"""
        B, P, b, lib = self.B, _ptr, self._b, _lib.load()
        C, hidden = x.shape[-1], blk_a.cSE[1].weight.shape[0]
        if blk_b.cSE[1].weight.shape[0] != hidden:
            raise ValueError(f"{tag}: the two SCSEBlocks differ in their reduction")

        def params(blk):
            return [P(t) for t in (blk.cSE[1].weight, blk.cSE[1].bias, blk.cSE[3].weight, blk.cSE[3].bias, blk.sSE[0].weight, blk.sSE[0].bias)]
        y = b.buf(f"{tag}.y", B, H, W, C)
        if lib.vp_scse2_preferred(B, H * W, C, hidden):
            ys = None
            if self.precision == "bf16x3" and C % 8 == 0:
                ys = b.sbuf(f"{tag}.ys", y.numel())
                self._planes[y.data_ptr()] = ys
            ws = b.ws(f"{tag}.scse2ws", lib.vp_scse2_workspace_bytes(B, H * W, C, hidden))
            plan.add("vp_scse2_fwd_f32", P(x), *params(blk_a), *params(blk_b), P(y), P(ys), B, H * W, C, hidden, 1, P(ws), ws.numel() * 4,
                     tag=f"{tag}.scse2")
            return y
        mid = b.buf(f"{tag}.mid", B, H, W, C)
        pool, hid, cg, sg = b.buf(f"{tag}.pool", B, C), b.buf(f"{tag}.hid", B, hidden), b.buf(f"{tag}.cgate", B, C), b.buf(f"{tag}.sgate", B, H * W)
        ws = b.ws(f"{tag}.scsews", lib.vp_scse_workspace_bytes(B, H * W, C, hidden))
        for i, (blk, src, dst, relu) in enumerate(((blk_a, x, mid, 0), (blk_b, mid, y, 1))):
            plan.add("vp_scse_fwd_f32", P(src), *params(blk), P(dst), P(pool), P(hid), P(cg), P(sg), B, H * W, C, hidden, relu, P(ws),
                     ws.numel() * 4, tag=f"{tag}.scse.{i}")
        return y

    def _style_up(self, plan, prep, tag, up, x, H, W, skip_tag, skip_block, skip_src):
        """StyleUp: the transposed convolution's InstanceNorm + ReLU writes channels [0, C) of cat_convs.0's input, the skip block's
        InstanceNorm writes [C, 2C); cat_convs.0 is one gather with bias and ReLU; then the SCSE pair"""
        B, P, b, lib = self.B, _ptr, self._b, _lib.load()
        ct = up.up_convs[0]
        C = ct.weight.shape[1]
        H2, W2 = 2 * H, 2 * W
        t = b.buf(f"{tag}.up_convs.0.y", B, H2, W2, C)
        self._scatter(plan, prep, f"{tag}.up_convs.0", ct, x, H, W, t)
        cat_in = b.buf(f"{tag}.cat.x", B, H2, W2, 2 * C)
        mean, rstd = b.buf(f"{tag}.up.mean", B, C), b.buf(f"{tag}.up.rstd", B, C)
        ws = b.ws(f"{tag}.up.inws", lib.vp_instnorm_workspace_bytes(B, H2 * W2, C))
        plan.add("vp_instnorm_act_fwd_ld_f32", P(t), P(cat_in), 2 * C, P(mean), P(rstd), B, H2 * W2, C, _IN_EPS, ops.ACT_RELU, 0.0, P(ws),
                 ws.numel() * 4, tag=f"{tag}.up_convs.in")
        self._in_conv(plan, prep, skip_tag, skip_block, skip_src, H2, W2, out=cat_in, ldy=2 * C, first_channel=C)
        v, _, _ = self._bias_conv(plan, prep, f"{tag}.cat_convs.0", up.cat_convs[0], cat_in, H2, W2)
        return self._scse_pair(plan, f"{tag}.cat_convs", up.cat_convs[1], up.cat_convs[2], v, H2, W2), H2, W2

    def _build_generator_body(self, mode, prep):
        """conv1 .. final of one label mode, reading ``self.g_in`` [B][S][S][4]; returns (plan, the NCHW result)"""
        G, B, S, P, b, lib = self.generator, self.B, self.S, _ptr, self._b, _lib.load()
        plan = _Plan()
        t = f"gen.{mode}"
        x, H, W = self._my_conv(plan, prep, f"{t}.conv1", G.conv1, mode, self.g_in, S, S)
        x, H, W = self._my_conv(plan, prep, f"{t}.conv2", G.conv2, mode, x, H, W)
        downs = []
        for k in range(1, 5):
            x, H, W = self._my_conv(plan, prep, f"{t}.down{k}", getattr(G, f"down{k}"), mode, x, H, W)
            downs.append(x)
        d1, d2, d3, _ = downs
        for k, skip_src in ((1, d3), (2, d2), (3, d1)):
            x, H, W = self._style_up(plan, prep, f"{t}.up{k}", getattr(G, f"up{k}"), x, H, W, f"{t}.skip{k}", getattr(G, f"skip{k}"), skip_src)
        f0 = b.buf(f"{t}.final.0.y", B, 2 * H, 2 * W, G.final[0].weight.shape[1])
        self._scatter(plan, prep, f"{t}.final.0", G.final[0], x, H, W, f0)
        x, H, W = self._bias_conv(plan, prep, f"{t}.final.1", G.final[1], f0, 2 * H, 2 * W)
        x, H, W = self._bias_conv(plan, prep, f"{t}.final.2", G.final[2], x, H, W)
        last = G.final[3].conv[0]
        cw = x.shape[-1]
        out = b.buf(f"{t}.out", B, 3, S, S)
        if tuple(last.weight.shape) == (3, cw, 3, 3) and lib.vp_sg_out_tanh_preferred(B, H, W, cw):
            par = b.buf(f"{t}.final.3.params", lib.vp_sg_out_params_floats(cw))
            prep.add("vp_sg_out_pack_f32", P(last.weight), P(last.bias), P(par), cw, tag=f"{t}.final.3.pack")
            plan.add("vp_sg_out_tanh_f32", P(x), P(par), P(out), B, H, W, cw, tag=f"{t}.final.3.tanh")
        else:
            y = b.buf(f"{t}.final.3.y", B, H, W, 3)
            prec, self.precision = self.precision, "f32"            # three output channels: the exact-fp32 entry
            try:
                self._gather(plan, prep, f"{t}.final.3", last.weight, last.bias, x, H, W, 3, cw, 3, 1, ops.ACT_NONE, y)
            finally:
                self.precision = prec
            plan.add("vp_act_fwd_f32", P(y), P(y), y.numel(), ops.ACT_TANH, 0.0, tag=f"{t}.final.3.act")
            plan.add("vp_nhwc_to_nchw_f32", P(y), P(out), B, 3, H, W, tag=f"{t}.final.3.nchw")
        return plan, out

    def _build_mlp(self, prep):
        """z -> the style plane [B][S*S]: one dense launch over the folded map, or the three layers"""
        G, B, S, Z, b = self.generator, self.B, self.S, self.Z, self._b
        plan = _Plan()
        l1, l2, l3 = (blk.fc[0] for blk in G.mlp.model)
        mid = l2.weight.shape[0]
        self.folded = _mlp_fold_preferred(S, Z)
        if self.folded:
            w21, b21 = b.buf("gen.mlp.w21", mid, Z), b.buf("gen.mlp.b21", mid)
            w_eff, b_eff = b.buf("gen.mlp.w_eff", S * S, Z), b.buf("gen.mlp.b_eff", S * S)
            b.lin_dgrad(prep, l2.weight, l1.weight, w21, mid, Z, Z)                 # W2 W1
            b.lin_fwd(prep, l1.bias, l2.weight, l2.bias, b21, 1, mid, Z)            # W2 b1 + b2
            b.lin_dgrad(prep, l3.weight, w21, w_eff, S * S, mid, Z)                 # W3 (W2 W1)
            b.lin_fwd(prep, b21, l3.weight, l3.bias, b_eff, 1, S * S, mid)          # W3 (W2 b1 + b2) + b3
            for c in prep.calls[-4:]:
                c[5] = "gen.mlp.fold"
            self._dense(plan, "gen.mlp.folded", SimpleNamespace(weight=w_eff, bias=b_eff), self.z, self.style)
        else:
            h1, h2 = b.buf("gen.mlp.h1", B, Z), b.buf("gen.mlp.h2", B, mid)
            for i, (lin, src, dst) in enumerate(((l1, self.z, h1), (l2, h1, h2), (l3, h2, self.style))):
                self._dense(plan, f"gen.mlp.model.{i}", lin, src, dst)
        return plan

    def _build_encoder(self, prep):
        E, B, S, Z, P, b = self.style_encoder, self.B, self.S, self.Z, _ptr, self._b
        plan = _Plan()
        convs = list(E.convs)
        x, H, W = self._bias_conv(plan, prep, "enc.convs.0", convs[0], self.xs_nhwc, S, S)
        for i, blk in enumerate(convs[1:-2], start=1):
            x, H, W = self._in_conv(plan, prep, f"enc.convs.{i}", blk, x, H, W)
        for i in (len(convs) - 2, len(convs) - 1):
            x, H, W = self._bias_conv(plan, prep, f"enc.convs.{i}", convs[i], x, H, W)
        assert (H, W) == (1, 1), (H, W)
        fm, fl = E.fc_mu.fc[0], E.fc_logvar.fc[0]
        wfc, bfc = self._stacked("enc.fc.w", (fm.weight, fl.weight)), self._stacked("enc.fc.b", (fm.bias, fl.bias))
        ml = b.buf("enc.fc.y", B, 2 * Z)
        self._dense(plan, "enc.fc", SimpleNamespace(weight=wfc, bias=bfc), x, ml)
        self.mu, self.logvar = b.buf("enc.mu", B, Z), b.buf("enc.logvar", B, Z)
        plan.add("vp_slice_channels_f32", P(ml), P(self.mu), B, 2 * Z, Z, tag="enc.mu")
        plan.add("vp_slice_channels_f32", _slice(ml, Z), P(self.logvar), B, 2 * Z, Z, tag="enc.logvar")
        return plan

    def _build_discriminator(self, prep):
        D, B, S, P, b = self.discriminator, self.B, self.S, _ptr, self._b
        plan = _Plan()
        convs = list(D.convs)
        x, H, W = self._bias_conv(plan, prep, "dis.convs.0", convs[0], self.d_in, S, S)
        for i, blk in enumerate(convs[1:], start=1):
            x, H, W = self._in_conv(plan, prep, f"dis.convs.{i}", blk, x, H, W)
        assert (H, W) == (4, 4), (H, W)
        ha, _, _ = self._bias_conv(plan, prep, "dis.adv_convs.0", D.adv_convs[0], x, H, W)
        hu, _, _ = self._bias_conv(plan, prep, "dis.aux_convs.0", D.aux_convs[0], x, H, W)
        pa, pu = D.adv_convs[1].conv[0], D.aux_convs[1].conv[0]
        self.adv, self.aux = b.buf("dis.adv", B, 1), b.buf("dis.aux", B, self.K)
        plan.add("vp_twin_head_fwd_f32", P(ha), P(hu), P(pa.weight), P(pa.bias), P(pu.weight), P(pu.bias), P(self.adv), P(self.aux), B,
                 ha.shape[-1], self.K, tag="dis.twin_head")
        return plan

    def _build(self):
        B, S, Z, P = self.B, self.S, self.Z, _ptr
        b = self._b = PlanBuilder(self, self.dev, self.precision, side_on=False, wgrad_cus=(0, 0))
        prep = _Plan()
        # x_content and the style / scored image, each in either memory layout
        self.xc_nchw, self.xc_nhwc = b.buf("xc_nchw", B, 3, S, S), b.buf("xc_nhwc", B, S, S, 3)
        self.xs_nchw, self.xs_nhwc = b.buf("xs_nchw", B, 3, S, S), b.buf("xs_nhwc", B, S, S, 3)
        self.z, self.eps, self.label = b.buf("z", B, Z), b.buf("eps", B, Z), b.buf("label", B)
        self.style, self.g_in = b.buf("gen.style", B, S * S), b.buf("gen.in", B, S, S, 4)

        p_mlp = self._build_mlp(prep)
        cat = {}
        for cl in (0, 1):
            cat[cl] = _Plan()
            cat[cl].add("vp_cat2_nhwc_f32", P(self.xc_nhwc if cl else self.xc_nchw), cl, P(self.style), 0, P(self.g_in), B, S * S, 3, 1,
                        tag="gen.in")
        self.out = {}
        body = {}
        for mode in _MODES:
            body[mode], self.out[mode] = self._build_generator_body(mode, prep)
        self._plans = {}
        for mode in _MODES:
            for cl in (0, 1):
                self._plans[f"generate.{mode}" + (".cl" if cl else "")] = (p_mlp, cat[cl], body[mode])

        if self.style_encoder is not None:
            to_nhwc = _Plan()
            to_nhwc.add("vp_nchw_to_nhwc_f32", P(self.xs_nchw), P(self.xs_nhwc), B, 3, S, S, tag="xs.nhwc")
            p_enc = self._build_encoder(prep)
            z_mu, z_eps = _Plan(), _Plan()
            z_mu.add("vp_slice_channels_f32", P(self._bufs["enc.fc.y"]), P(self.z), B, 2 * Z, Z, tag="z.mu")
            z_eps.add("vp_latent_fwd_f32", P(self.mu), P(self.logvar), P(self.eps), P(self.z), None, B, Z, tag="z.latent")
            for cl in (0, 1):
                enc = (p_enc,) if cl else (to_nhwc, p_enc)
                self._plans["encode" + (".cl" if cl else "")] = enc
                for mode in _MODES:
                    for with_eps, p_z in ((0, z_mu), (1, z_eps)):
                        name = f"stylize.{mode}" + (".eps" if with_eps else "") + (".cl" if cl else "")
                        self._plans[name] = enc + (p_z,) + self._plans[f"generate.{mode}" + (".cl" if cl else "")]

        if self.discriminator is not None:
            self.d_in = b.buf("dis.in", B, S, S, 6)
            p_dis = self._build_discriminator(prep)
            for cl in (0, 1):
                p_cat = _Plan()
                p_cat.add("vp_cat2_nhwc_f32", P(self.xs_nhwc if cl else self.xs_nchw), cl, P(self.xc_nhwc if cl else self.xc_nchw), cl,
                          P(self.d_in), B, S * S, 3, 3, tag="dis.in")
                self._plans["discriminate" + (".cl" if cl else "")] = (p_cat, p_dis)
        b.dense_workspace()
        self._prep = prep
        self._n_side_events = 0

    # ---- execution ---------------------------------------------------------------------------
    def refresh(self) -> None:
        """Re-read the modules: stack the paired weights and the two fc heads, pack every convolution weight, fold ``mlp``.  Runs when
        the plan is built; call it again after a module's parameters changed.  Graphs captured before are captured again."""
        with torch.no_grad():
            for dst, srcs in self._stacks:
                r = 0
                for t in srcs:
                    dst[r:r + t.shape[0]].copy_(t)
                    r += t.shape[0]
        self._prep.run(torch.cuda.current_stream().cuda_stream)
        if self._graphs:
            self._graphs = {}
            self.capture()

    def capture(self, warmup: int = 2):
        """Capture every launch list into one hipGraph each and replay them from then on; the results are bit-identical to the eager
        launches."""
        self._graphs = self._capture(list(self._plans), warmup)
        return self._graphs

    def _check(self, t, what: str, tail) -> None:
        shape = f"(n, {', '.join(map(str, tail))})"
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.VaePlayHipError(f"FusedStyleGanInference: {what} must be a tensor of shape {shape} on the HIP device (no CPU path exists)")
        if t.dtype != torch.float32:
            raise _lib.VaePlayHipError(f"FusedStyleGanInference: {what} must be fp32 of shape {shape}, got {t.dtype}")
        if t.dim() != len(tail) + 1 or tuple(t.shape[1:]) != tuple(tail) or t.shape[0] == 0:
            raise _lib.VaePlayHipError(f"FusedStyleGanInference: {what} has shape {tuple(t.shape)}, this plan takes {shape}")

    def _need(self, net, method: str, what: str):
        if net is None:
            raise _lib.VaePlayHipError(f"FusedStyleGanInference: {method}() needs the {what}, this plan was built without one")

    @staticmethod
    def _is_cl(x) -> bool:
        return x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()

    def _image(self, x, what: str, nchw, nhwc, cl: Optional[bool] = None, n: Optional[int] = None):
        """validate an image batch; returns (channels_last?, (static buffer, source)) in the layout ``cl`` (default: the tensor's own)"""
        self._check(x, what, (3, self.S, self.S))
        if n is not None and x.shape[0] != n:
            raise _lib.VaePlayHipError(f"FusedStyleGanInference: {what} has shape {tuple(x.shape)}, the other inputs have {n} rows: this "
                                       f"plan takes (n, 3, {self.S}, {self.S}) with the same n")
        if cl is None:
            cl = self._is_cl(x)
        if cl:
            return True, (nhwc, x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1))
        return False, (nchw, x.contiguous())

    def _labels(self, labels, n: int):
        """(list infix, the load of the label buffer or None)"""
        if isinstance(labels, bool) or (isinstance(labels, int) and labels not in (0, 1)):
            raise _lib.VaePlayHipError("FusedStyleGanInference: labels must be a tensor of shape (n,), a float, or the int 0 or 1")
        if isinstance(labels, int):
            return f"c{labels}", None
        if isinstance(labels, float):
            return "blend", (self.label, torch.full((n,), labels, dtype=torch.float32, device=self.dev))
        if not isinstance(labels, torch.Tensor) or labels.numel() != n:
            raise _lib.VaePlayHipError(f"FusedStyleGanInference: labels must have one element per image: this plan takes (n,) with n = {n}")
        return "blend", (self.label, labels.detach().reshape(-1).to(device=self.dev, dtype=torch.float32))

    def _generate(self, which: str, mode: str, n: int, loads, like):
        out = like.new_empty((n, 3, self.S, self.S))
        for i0, m in self._chunks(n):
            for static, src in loads:
                self._load(static, src[i0:i0 + m])
            self._run(which)
            out[i0:i0 + m].copy_(self.out[mode][:m])
        return out

    def generate(self, x_content: torch.Tensor, z: torch.Tensor, labels) -> torch.Tensor:
        """(n, 3, S, S) = ``generator(x_content, z, labels)``.  ``labels``: one number per image (a tensor of any dtype, or a Python
        float for all of them) runs the blended lists; the Python int 0 or 1 runs that class's branch alone."""
        cl, load_x = self._image(x_content, "x_content", self.xc_nchw, self.xc_nhwc)
        n = x_content.shape[0]
        self._check(z, "z", (self.Z,))
        if z.shape[0] != n:
            raise _lib.VaePlayHipError(f"FusedStyleGanInference: z has shape {tuple(z.shape)}, x_content has {n} rows: this plan takes "
                                       f"(n, {self.Z}) with the same n")
        mode, load_l = self._labels(labels, n)
        loads = [load_x, (self.z, z.contiguous())] + ([load_l] if load_l else [])
        return self._generate(f"generate.{mode}" + (".cl" if cl else ""), mode, n, loads, x_content)

    def encode_style(self, x: torch.Tensor):
        """(mu, logvar), each (n, z_dim) = ``style_encoder(x)``"""
        self._need(self.style_encoder, "encode_style", "style encoder")
        cl, load_x = self._image(x, "x", self.xs_nchw, self.xs_nhwc)
        n = x.shape[0]
        mu, logvar = x.new_empty((n, self.Z)), x.new_empty((n, self.Z))
        for i0, m in self._chunks(n):
            self._load(load_x[0], load_x[1][i0:i0 + m])
            self._run("encode" + (".cl" if cl else ""))
            mu[i0:i0 + m].copy_(self.mu[:m])
            logvar[i0:i0 + m].copy_(self.logvar[:m])
        return mu, logvar

    def stylize(self, x_content: torch.Tensor, x_style: torch.Tensor, labels, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``generator(x_content, z, labels)`` with z from ``style_encoder(x_style)`` in one launch list: z = mu, or with ``eps``
        (n, z_dim) z = mu + eps exp(logvar / 2) (train_Style_GAN.py:156-160)"""
        self._need(self.style_encoder, "stylize", "style encoder")
        cl, load_c = self._image(x_content, "x_content", self.xc_nchw, self.xc_nhwc)
        n = x_content.shape[0]
        _, load_s = self._image(x_style, "x_style", self.xs_nchw, self.xs_nhwc, cl=cl, n=n)
        mode, load_l = self._labels(labels, n)
        loads = [load_c, load_s] + ([load_l] if load_l else [])
        if eps is not None:
            self._check(eps, "eps", (self.Z,))
            if eps.shape[0] != n:
                raise _lib.VaePlayHipError(f"FusedStyleGanInference: eps has shape {tuple(eps.shape)}, x_content has {n} rows: this plan "
                                           f"takes (n, {self.Z}) with the same n")
            loads.append((self.eps, eps.contiguous()))
        which = f"stylize.{mode}" + (".eps" if eps is not None else "") + (".cl" if cl else "")
        return self._generate(which, mode, n, loads, x_content)

    def discriminate(self, x: torch.Tensor, x_content: torch.Tensor):
        """(adv (n, 1), aux (n, num_of_classes)) = ``discriminator(x, x_content, y)`` (the reference's unused ``y`` is not taken)"""
        self._need(self.discriminator, "discriminate", "discriminator")
        cl, load_x = self._image(x, "x", self.xs_nchw, self.xs_nhwc)
        n = x.shape[0]
        _, load_c = self._image(x_content, "x_content", self.xc_nchw, self.xc_nhwc, cl=cl, n=n)
        adv, aux = x.new_empty((n, 1)), x.new_empty((n, self.K))
        for i0, m in self._chunks(n):
            for static, src in (load_x, load_c):
                self._load(static, src[i0:i0 + m])
            self._run("discriminate" + (".cl" if cl else ""))
            adv[i0:i0 + m].copy_(self.adv[:m])
            aux[i0:i0 + m].copy_(self.aux[:m])
        return adv, aux
