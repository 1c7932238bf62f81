"""Fused inference for the font U-Net ``networks_BE_font.ComposeNet``: what the reference's ``test_BE_font.py:99`` does -- ``net.eval()``,
``net(imgs)``, threshold the two maps (test_BE_font.py:27-31) -- as a fixed, pre-planned, hipGraph-replayable list of HIP launches.

  * a convolution + InstanceNorm + activation block whose output map has at most 256 pixels and whose K = k*k*Cin is at most 576 is ONE
    launch of the whole-image kernel (csrc/font_infer.hip): a workgroup holds whole images, so the per-(image, channel) statistics come
    from its accumulators;
  * the other InstanceNorm blocks (larger maps, a 3-channel input, a longer K -- where the kernel was measured slower than the pair) are
    the existing convolution plus one InstanceNorm entry;
  * every convolution + BatchNorm + ReLU block (``down.k.0``, both layers of each ``Up``) is ONE launch of the existing convolution with
    the eval-mode BatchNorm folded into weight and bias, as ``FusedBEInference`` does for ``aux_convs``;
  * ``torch.cat`` never runs: the 2x resize of ``Up`` and the ``skip`` block each write their channel slice of the ``cat`` block's input;
  * the relay input row is one small kernel, the two heads' last convolutions are one launch that also writes the thresholded masks.

``precision`` selects the arithmetic of the layers on the existing convolution entry only -- "f32" (exact fp32 products) or "bf16x3"
(split-bf16 operands; layers with a 3-channel input stay exact fp32); the new kernels are always exact fp32.  DESIGN.md 11.1.
"""
from __future__ import annotations

from ctypes import c_void_p
from typing import Dict, Optional

import torch

from . import _lib, networks_BE_font, ops, seg_eval
from .infer import FusedVAEInference
from .plan import PlanBuilder, _Plan, _ptr, plan_device

_HEADS = ("edges", "masks")     # head 0, head 1 of every stacked buffer
_IN_EPS = 1e-5                  # blocks._InstanceNormActM: nn.InstanceNorm2d's default
_N_CLS, _N_STYLE = networks_BE_font._N_CLASSES, networks_BE_font._N_STYLE
_EMBED = networks_BE_font.LABEL_EMBED


def _bn_args(bn):
    return (_ptr(bn.weight), _ptr(bn.bias), _ptr(bn.running_mean), _ptr(bn.running_var))


def _slice(t: torch.Tensor, first_channel: int):
    """launch argument of a channel slice of an NHWC buffer: the address of its first element"""
    return c_void_p(t.data_ptr() + 4 * first_channel)


class FusedFontInference:
    """``predict`` / ``segment`` / ``condition`` of a ``networks_BE_font.ComposeNet`` on (n, 3, S, S) fp32 images, contiguous or
    channels_last; ``y`` = None conditions on the image through ``style_encoder`` (what test_BE_font.py runs), ``y`` = {"cls": (n, 143),
    "cnt_style": (n, 5)} through ``embeding_block``.

    The plan SNAPSHOTS the model when it is built: weights are folded and packed into plan-owned buffers once, not per call.  After the
    module's parameters or buffers change call ``refresh()``; until then the plan keeps computing with what it was built with.  Nothing
    here writes to the module, ``net.training`` is left as found, and the result is eval-mode arithmetic (running statistics) whatever
    the mode.  Inputs of any number of images run in chunks of ``batch_size``; a short last chunk is padded with zero images."""

    _run, _capture, _chunks = FusedVAEInference._run, FusedVAEInference._capture, FusedVAEInference._chunks
    _load = staticmethod(FusedVAEInference._load)

    def __init__(self, net, batch_size: int, precision: str = "f32", _plan_only: bool = False):
        if precision not in ("f32", "bf16x3"):
            raise ValueError("precision must be 'f32' or 'bf16x3'")
        if not isinstance(net, networks_BE_font.ComposeNet):
            raise ValueError("FusedFontInference takes a networks_BE_font.ComposeNet")
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self.net, self.precision = net, precision
        self.levels = len(net.down) - 1
        self.S = 4 * 2 ** self.levels
        self.B = int(batch_size)
        self.dev = plan_device(net, "FusedFontInference", _plan_only)
        self._bufs: Dict[str, torch.Tensor] = {}
        self._graphs: Dict[str, "torch.cuda.CUDAGraph"] = {}
        self._planes: Dict[int, torch.Tensor] = {}
        self._build()
        if not _plan_only:
            self.refresh()

    # ---- plan construction: one emitter per kind of block ---------------------------------------------------------------------
    def _split_of(self, plan, tag, t):
        """the bf16 planes of fp32 buffer ``t``: those its producer wrote, else one vp_split_f32 launch here"""
        s = self._planes.get(t.data_ptr())
        if s is None:
            s = self._b.sbuf(f"{tag}.xs", t.numel())
            plan.add("vp_split_f32", _ptr(t), _ptr(s), t.numel(), tag=f"{tag}.split")
            self._planes[t.data_ptr()] = s          # (a later reader in the same list takes these)
        return s

    def _gather(self, plan, prep, tag, weight, bias, src, H, W, cout, cin, ks, stride, act, out):
        """the existing k x k convolution entry in the plan's arithmetic: out = act(conv(src) + bias)"""
        B, P = self.B, _ptr
        pad = (ks - 1) // 2
        Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        geom = (B, Ho, Wo, H, W, cin, cout, ks, stride, act)
        flops = 2.0 * B * Ho * Wo * cin * cout * ks * ks
        if self.precision == "bf16x3" and cin % 8 == 0:
            p0 = self._b.sbuf(f"{tag}.p0s", cout * cin * ks * ks)
            prep.add("vp_pack_w_split", P(weight), P(p0), None, cout, cin, ks, tag=f"{tag}.pack")
            xs = self._split_of(plan, tag, src)
            plan.add("vp_conv_gather_bf16x3", P(xs), P(p0), P(bias), P(out), *geom, flops=flops, tag=f"{tag}.fwd")
        else:
            p0 = self._b.buf(f"{tag}.p0", cout, ks * ks, cin)
            prep.add("vp_pack_w_f32", P(weight), P(p0), None, cout, cin, ks, tag=f"{tag}.pack")
            plan.add("vp_conv_gather_f32", P(src), P(p0), P(bias), P(out), *geom, flops=flops, tag=f"{tag}.fwd")
        return Ho, Wo

    def _bn_conv(self, plan, prep, tag, block, src, H, W):
        """convolution + eval-mode BatchNorm + ReLU as ONE launch: the folded scale in the weight, the folded shift as the bias"""
        conv, bn = block.conv[0], block.conv[1]
        if bn.act != "relu":
            raise ValueError(f"{tag}: the gather epilogue takes ReLU, the block has {bn.act}")
        cout, cin, ks = conv.weight.shape[0], conv.weight.shape[1], conv.kernel_size
        wf, shift = self._b.buf(f"{tag}.wf", cout, cin, ks, ks), self._b.buf(f"{tag}.shift", cout)
        prep.add("vp_be_fold_conv_f32", _ptr(conv.weight), *_bn_args(bn), float(bn.eps), _ptr(wf), _ptr(shift), cout, cin * ks * ks,
                 tag=f"{tag}.fold")
        pad = (ks - 1) // 2
        Ho, Wo = (H + 2 * pad - ks) // conv.stride + 1, (W + 2 * pad - ks) // conv.stride + 1
        out = self._b.buf(f"{tag}.y", self.B, Ho, Wo, cout)
        self._gather(plan, prep, tag, wf, shift, src, H, W, cout, cin, ks, conv.stride, ops.ACT_RELU, out)
        return out, Ho, Wo

    def _in_conv(self, plan, prep, tag, block, src, H, W, out=None, ldy=0, first_channel=0):
        """convolution + InstanceNorm + activation: ONE launch of the whole-image kernel where vp_conv_in_preferred names the layer
        (the supported shapes it was measured faster on), else the existing convolution and one InstanceNorm entry.  ``out`` / ``ldy`` / ``first_channel``: a channel slice of a wider
        NHWC buffer (a concatenation's input) instead of a buffer of the layer's own."""
        B, P, b, lib = self.B, _ptr, self._b, _lib.load()
        conv, norm = block.conv[0], block.conv[1]
        cout, cin, ks, stride = conv.weight.shape[0], conv.weight.shape[1], conv.kernel_size, conv.stride
        act, slope = ops.ACT_CODES[norm.act], float(norm.slope)
        if act not in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU):
            raise ValueError(f"{tag}: activation {norm.act} is not one the fused InstanceNorm blocks take")
        pad = (ks - 1) // 2
        Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        if out is None:
            out, ldy = b.buf(f"{tag}.y", B, Ho, Wo, cout), cout
        dense = ldy == cout
        dst = _slice(out, first_channel)
        if lib.vp_conv_in_preferred(H, W, cin, cout, ks, stride):
            wp = b.buf(f"{tag}.wp", cout, ks * ks, cin)
            prep.add("vp_conv_in_pack_f32", P(conv.weight), P(wp), cout, cin, ks, tag=f"{tag}.pack")
            plan.add("vp_conv_in_act_f32", P(src), P(wp), dst, ldy, B, H, W, cin, cout, ks, stride, _IN_EPS, act, slope,
                     flops=2.0 * B * Ho * Wo * cin * cout * ks * ks, tag=f"{tag}.fwd")
            return out, Ho, Wo
        c = b.buf(f"{tag}.c", B, Ho, Wo, cout)
        self._gather(plan, prep, tag, conv.weight, None, src, H, W, cout, cin, ks, stride, ops.ACT_NONE, c)
        R = Ho * Wo
        mean, rstd = b.buf(f"{tag}.mean", B, cout), b.buf(f"{tag}.rstd", B, cout)
        ws = b.ws(f"{tag}.inws", lib.vp_instnorm_workspace_bytes(B, R, cout))
        tail = (B, R, cout, _IN_EPS, act, slope, P(ws), ws.numel() * 4)
        if not dense:
            plan.add("vp_instnorm_act_fwd_ld_f32", P(c), dst, ldy, P(mean), P(rstd), *tail, tag=f"{tag}.in")
        elif self.precision == "bf16x3" and cout % 8 == 0:
            ys = b.sbuf(f"{tag}.ys", out.numel())
            self._planes[out.data_ptr()] = ys
            plan.add("vp_instnorm_act_fwd_split_f32", P(c), P(out), P(ys), P(mean), P(rstd), *tail, tag=f"{tag}.in")
        else:
            plan.add("vp_instnorm_act_fwd_f32", P(c), P(out), P(mean), P(rstd), *tail, tag=f"{tag}.in")
        return out, Ho, Wo

    def _dense(self, plan, tag, lin, x, y, act=None, slope=0.0):
        """Linear (+ activation in place) on the dense path the modules use"""
        N, K = lin.weight.shape
        self._b.lin_fwd(plan, x, lin.weight, lin.bias, y, self.B, N, K)
        plan.calls[-1][5] = f"{tag}.fwd"
        if act is not None:
            plan.add("vp_act_fwd_f32", _ptr(y), _ptr(y), y.numel(), ops.ACT_CODES[act], float(slope), tag=f"{tag}.act")

    def _embed_block(self, plan, tag, blk, x, out):
        """EmbedingBlock on (B, width) rows: on a 1 x 1 map the attention is gamma relu(W_v x + b_v) + x (q and k drop out)"""
        B, b = self.B, self._b
        width = blk.convs_first[0].fc[0].weight.shape[0]
        h0, h1, v = (b.buf(f"{tag}.{n}", B, width) for n in ("h0", "h1", "v"))
        self._dense(plan, f"{tag}.convs_first.0", blk.convs_first[0].fc[0], x, h0)
        self._dense(plan, f"{tag}.convs_first.1", blk.convs_first[1].fc[0], h0, h1)
        for i, att in enumerate(blk.attention):
            vc = att.v.conv[0]
            b.lin_fwd(plan, h1, vc.weight, vc.bias, v, B, width, width)         # the 1x1 convolution's (C, C, 1, 1) weight is [C][C]
            plan.calls[-1][5] = f"{tag}.attention.{i}.v"
            plan.add("vp_font_attn1_f32", _ptr(v), _ptr(h1), _ptr(att.gamma), _ptr(h1), B * width, tag=f"{tag}.attention.{i}.out")
        e0, e1 = blk.embeding[0], blk.embeding[1]
        self._dense(plan, f"{tag}.embeding.0", e0.fc[0], h1, h0, e0.fc[1].act, e0.fc[1].slope)
        self._dense(plan, f"{tag}.embeding.1", e1.fc[0], h0, out, e1.fc[1].act, e1.fc[1].slope)

    def _style_block(self, plan, prep, tag, blk, x, out):
        """StyleEncodeBlock: the InstanceNorm ladder down to 4 x 4, the 1x1 projection, the global average"""
        H = W = self.S
        layers = list(blk.convs)
        for i, layer in enumerate(layers[:-1]):
            x, H, W = self._in_conv(plan, prep, f"{tag}.convs.{i}", layer, x, H, W)
        plan.add("vp_global_avgpool_fwd_f32", _ptr(x), _ptr(out), self.B, H * W, x.shape[-1], tag=f"{tag}.pool")

    def _build(self):
        net, B, S, L, P = self.net, self.B, self.S, self.levels, _ptr
        lib = _lib.load()
        b = self._b = PlanBuilder(self, self.dev, self.precision, side_on=False, wgrad_cus=(0, 0))
        prep, to_nhwc, p_img, p_emb, p_body, p_pred, p_seg = (_Plan() for _ in range(7))

        self.x_nchw, self.x_nhwc = b.buf("x_nchw", B, 3, S, S), b.buf("x_nhwc", B, S, S, 3)
        self.y_cls, self.y_sty = b.buf("y_cls", B, _N_CLS), b.buf("y_sty", B, _N_STYLE)
        self.label, self.style = b.buf("label", B, _EMBED), b.buf("style", B, _EMBED)
        to_nhwc.add("vp_nchw_to_nhwc_f32", P(self.x_nchw), P(self.x_nhwc), B, 3, S, S, tag="x.nhwc")

        # ---- the two conditioning branches: both leave (label, style) where the relay input reads them ----
        self._style_block(p_img, prep, "style_encoder.label_encode_block", net.style_encoder.label_encode_block, self.x_nhwc, self.label)
        self._style_block(p_img, prep, "style_encoder.style_encode_block", net.style_encoder.style_encode_block, self.x_nhwc, self.style)
        self._embed_block(p_emb, "embeding_block.label_encode_block", net.embeding_block.label_encode_block, self.y_cls, self.label)
        self._embed_block(p_emb, "embeding_block.style_encode_block", net.embeding_block.style_encode_block, self.y_sty, self.style)

        # ---- encoder ladder ----
        x, H, W = self._in_conv(p_body, prep, "down.0", net.down[0], self.x_nhwc, S, S)
        pyramid = [(x, H, W)]
        for k in range(1, L + 1):
            x, H, W = self._bn_conv(p_body, prep, f"down.{k}.0", net.down[k][0], x, H, W)
            x, H, W = self._in_conv(p_body, prep, f"down.{k}.1", net.down[k][1], x, H, W)
            pyramid.append((x, H, W))

        # ---- dense bottleneck: [map in (C,H,W) order | label | style] -> two Linear + ReLU -> back to NHWC ----
        C = x.shape[-1]
        flat = C * H * W
        r_in, r0, r1 = b.buf("relay.in", B, flat + 2 * _EMBED), b.buf("relay.0.y", B, flat), b.buf("relay.1.y", B, flat)
        p_body.add("vp_font_relay_input_f32", P(x), P(self.label), P(self.style), P(r_in), B, H * W, C, _EMBED, tag="relay.in")
        for i, (src, dst) in enumerate(((r_in, r0), (r0, r1))):
            fc = net.relay_convs[i].fc
            self._dense(p_body, f"relay_convs.{i}", fc[0], src, dst, fc[1].act, fc[1].slope)
        x = b.buf("relay.nhwc", B, H, W, C)
        p_body.add("vp_nchw_to_nhwc_f32", P(r1), P(x), B, C, H, W, tag="relay.nhwc")

        # ---- decoder: Up writes channels [0, narrow) of the cat block's input, skip writes [narrow, 2 narrow) ----
        for k in reversed(range(L)):
            u, _, _ = self._bn_conv(p_body, prep, f"up.{k}.conv.0", net.up[k].conv[0], x, H, W)
            u, _, _ = self._bn_conv(p_body, prep, f"up.{k}.conv.1", net.up[k].conv[1], u, H, W)
            narrow = u.shape[-1]
            cat_in = b.buf(f"cat.{k}.x", B, 2 * H, 2 * W, 2 * narrow)
            p_body.add("vp_upsample2x_bilinear_fwd_ld_f32", P(u), P(cat_in), 2 * narrow, B, H, W, narrow, tag=f"up.{k}.resize")
            sk, sh, sw = pyramid[k]
            assert (sh, sw, sk.shape[-1]) == (2 * H, 2 * W, narrow), (k, sh, sw, sk.shape)
            self._in_conv(p_body, prep, f"skip.{k}", net.skip[k], sk, sh, sw, out=cat_in, ldy=2 * narrow, first_channel=narrow)
            x, H, W = self._in_conv(p_body, prep, f"cat.{k}", net.cat[k], cat_in, 2 * H, 2 * W)

        # ---- the heads: two InstanceNorm blocks each, then ONE launch for both output convolutions (+ the masks) ----
        self.heads = (net.edge_net, net.mask_net)
        cw = x.shape[-1]
        n_pr = lib.vp_font_pred_params_floats(cw)
        if not n_pr:
            raise ValueError(f"the heads' output stage takes a multiple of 4 channels up to 256, the net has {cw}")
        par = b.buf("heads.pred.params", 2, n_pr)
        h0, h1 = b.buf("heads.h0", 2, B, S, S, cw), b.buf("heads.h1", 2, B, S, S, cw)
        for k, head in enumerate(self.heads):
            name = f"{_HEADS[k][:-1]}_net"
            self._in_conv(p_body, prep, f"{name}.predictor.0", head.predictor[0], x, S, S, out=h0[k], ldy=cw)
            self._in_conv(p_body, prep, f"{name}.predictor.1", head.predictor[1], h0[k], S, S, out=h1[k], ldy=cw)
            last = head.predictor[2].conv[0]
            prep.add("vp_font_pred_pack_f32", P(last.weight), P(last.bias), P(par[k]), cw, tag=f"{name}.predictor.2.pack")
        self.logits = b.buf("heads.logits", 2, B, 1, S, S)
        self.masks = torch.empty((2, B, 1, S, S), dtype=torch.uint8, device=self.dev)
        self._bufs["heads.masks"] = self.masks
        pred = (P(h1), h1[0].numel(), P(par), P(self.logits))
        p_pred.add("vp_font_pred_infer_f32", *pred, None, 0.0, 2, B, S, S, cw, tag="heads.pred")
        self._threshold = 0.5
        p_seg.add("vp_font_pred_infer_f32", *pred, P(self.masks), self._threshold, 2, B, S, S, cw, tag="heads.pred")
        self._seg_args = p_seg.calls[0][2]
        b.dense_workspace()
        self._prep = prep
        self._n_side_events = 0
        self._plans = {"condition": (to_nhwc, p_img), "condition.cl": (p_img,), "condition.y": (p_emb,)}
        for which, tail in (("predict", p_pred), ("segment", p_seg)):
            self._plans.update({which: (to_nhwc, p_img, p_body, tail), which + ".cl": (p_img, p_body, tail),
                                which + ".y": (to_nhwc, p_emb, p_body, tail), which + ".y.cl": (p_emb, p_body, tail)})

    # ---- execution ---------------------------------------------------------------------------
    def refresh(self) -> None:
        """Re-read the model: fold every BatchNorm, pack every convolution weight and the heads' parameter block.  Runs when the plan is
        built; call it again after the module's parameters or buffers changed.  Graphs captured before are captured again."""
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
            raise _lib.VaePlayHipError(f"FusedFontInference: {what} must be a tensor of shape {shape} on the HIP device (no CPU path exists)")
        if t.dtype != torch.float32:
            raise _lib.VaePlayHipError(f"FusedFontInference: {what} must be fp32 of shape {shape}, got {t.dtype}")
        if t.dim() != len(tail) + 1 or tuple(t.shape[1:]) != tuple(tail) or t.shape[0] == 0:
            raise _lib.VaePlayHipError(f"FusedFontInference: {what} has shape {tuple(t.shape)}, this plan takes {shape}")

    def _feed(self, x, y):
        """validate the inputs; returns (n, the list suffix, [(static buffer view, source), ...])"""
        loads, suffix, n = [], "", None
        if y is not None:
            if not isinstance(y, dict) or "cls" not in y or "cnt_style" not in y:
                raise _lib.VaePlayHipError(f"FusedFontInference: y must be None or a dict with 'cls' of shape (n, {_N_CLS}) and "
                                           f"'cnt_style' of shape (n, {_N_STYLE})")
            self._check(y["cls"], "y['cls']", (_N_CLS,))
            self._check(y["cnt_style"], "y['cnt_style']", (_N_STYLE,))
            n = y["cls"].shape[0]
            if y["cnt_style"].shape[0] != n:
                raise _lib.VaePlayHipError(f"FusedFontInference: y['cnt_style'] has shape {tuple(y['cnt_style'].shape)}, y['cls'] has "
                                           f"{n} rows: this plan takes (n, {_N_STYLE})")
            loads += [(self.y_cls, y["cls"].contiguous()), (self.y_sty, y["cnt_style"].contiguous())]
            suffix = ".y"
        if x is not None:
            self._check(x, "x", (3, self.S, self.S))
            if n is not None and x.shape[0] != n:
                raise _lib.VaePlayHipError(f"FusedFontInference: x has shape {tuple(x.shape)}, y has {n} rows: this plan takes "
                                           f"(n, 3, {self.S}, {self.S}) with the same n")
            n = x.shape[0]
            if x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
                loads.append((self.x_nhwc, x.permute(0, 2, 3, 1)))
                suffix += ".cl"
            else:
                loads.append((self.x_nchw, x.contiguous()))
        return n, suffix, loads

    def _heads_out(self, x, y, which, with_masks):
        if x is None:
            raise _lib.VaePlayHipError(f"FusedFontInference: x must be a tensor of shape (n, 3, {self.S}, {self.S}) on the HIP device")
        n, suffix, loads = self._feed(x, y)
        shape = (n, 1, self.S, self.S)
        out = {k: x.new_empty(shape) for k in _HEADS}
        if with_masks:
            out.update({k[:-1] + "_mask": torch.empty(shape, dtype=torch.bool, device=x.device) for k in _HEADS})
        for i0, m in self._chunks(n):
            for static, src in loads:
                self._load(static, src[i0:i0 + m])
            self._run(which + suffix)
            for k, name in enumerate(_HEADS):
                out[name][i0:i0 + m].copy_(self.logits[k, :m])
                if with_masks:
                    out[name[:-1] + "_mask"][i0:i0 + m].copy_(self.masks[k, :m])
        return out

    def predict(self, x: torch.Tensor, y: Optional[dict] = None) -> Dict[str, torch.Tensor]:
        """{"edges", "masks"}: the two heads' logits (n, 1, S, S), as ``net(x, y)`` returns them in eval mode"""
        return self._heads_out(x, y, "predict", False)

    def segment(self, x: torch.Tensor, y: Optional[dict] = None, threshold: float = 0.5) -> Dict[str, torch.Tensor]:
        """``predict`` plus "edge_mask" and "mask_mask" (torch.bool) = logits >= threshold (the reference thresholds the raw output,
        test_BE_font.py:27-31), written by the same launch as the logits"""
        threshold = float(threshold)
        if threshold != self._threshold:
            self._seg_args[5] = threshold
            self._threshold = threshold
            if self._graphs:
                self._graphs.update(self._capture([k for k in self._plans if k.startswith("segment")]))
        return self._heads_out(x, y, "segment", True)

    def evaluate(self, x: torch.Tensor, edge_targets: torch.Tensor, mask_targets: torch.Tensor, y: Optional[dict] = None,
                 threshold: float = 0.5, tolerance: int = 0, bce_weight: float = 0.5, smooth: float = 1.0) -> Dict[str, Dict[str, torch.Tensor]]:
        """{"edges": result, "masks": result}, each the ``seg_eval.segmentation_metrics`` result -- per-image loss terms of
        train_BE.py:58-59, confusion counts at ``threshold`` (``segment``'s rule), the boundary match within ``tolerance`` pixels -- of
        the images x (conditioned as ``predict`` does) against (n, 1, S, S) fp32 targets: every batch chunk runs the ``predict`` launch
        list and is evaluated where its logits lie in the plan, so nothing is copied out."""
        if x is None:
            raise _lib.VaePlayHipError(f"FusedFontInference: x must be a tensor of shape (n, 3, {self.S}, {self.S}) on the HIP device")
        rows = x.shape[0] if isinstance(x, torch.Tensor) and x.dim() == 4 else 0
        for t, what in ((edge_targets, "edge_targets"), (mask_targets, "mask_targets")):
            seg_eval.check_planes(t, what, rows or None, (self.S, self.S))
        n, suffix, loads = self._feed(x, y)

        def chunks():
            for i0, m in self._chunks(n):
                for static, src in loads:
                    self._load(static, src[i0:i0 + m])
                self._run("predict" + suffix)
                yield i0, m
        return seg_eval.evaluate_plan(self, n, chunks(), edge_targets, mask_targets, threshold, tolerance, bce_weight, smooth)

    def condition(self, x: Optional[torch.Tensor] = None, y: Optional[dict] = None):
        """(label, style), each (n, 256): ``embeding_block(y["cls"], y["cnt_style"])`` when ``y`` is given, else ``style_encoder(x, x)``"""
        if x is None and y is None:
            raise _lib.VaePlayHipError(f"FusedFontInference: condition() takes x of shape (n, 3, {self.S}, {self.S}) or y")
        n, suffix, loads = self._feed(None if y is not None else x, y)
        ref = y["cls"] if y is not None else x
        label, style = ref.new_empty((n, _EMBED)), ref.new_empty((n, _EMBED))
        for i0, m in self._chunks(n):
            for static, src in loads:
                self._load(static, src[i0:i0 + m])
            self._run("condition" + suffix)
            label[i0:i0 + m].copy_(self.label[:m])
            style[i0:i0 + m].copy_(self.style[:m])
        return label, style
