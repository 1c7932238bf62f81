"""Fused segmentation inference for the mask / edge heads of ``networks_BE`` / ``networks_BE_GAN``: what the reference's
``test_BE.py:92-98`` and ``test_BE_manga.py`` do below the backbone -- ``net.eval()``, ``net(imgs)``, threshold the two maps
(test_BE.py:35-39) -- as a fixed, pre-planned, hipGraph-replayable list of HIP launches with every eval-mode BatchNorm folded away.

  * each ``aux_convs`` layer (1x1 / 3x3 convolution + BatchNorm + ReLU, 256 -> 32 channels: MFMA work) is ONE launch of the existing
    k x k convolution with its weight pre-multiplied by the folded scale and the folded shift as its bias;
  * each ``Up`` block (AddCoords, two convolution + BatchNorm + ReLU pairs, 2x bilinear resize) is ONE launch for both heads
    (csrc/be_infer.hip): the coordinate channels are computed, both convolution outputs live in LDS;
  * the three bias-only predictor convolutions are ONE launch for both heads, which also writes the thresholded masks.

For a channels_last input that is ``len(aux_convs) + 3`` launches in an "f32" plan, where the module path in ``.eval()`` runs more
than forty.  ``precision`` selects the arithmetic of the ``aux_convs`` layers only -- "f32" (exact fp32 products) or
"bf16x3" (split-bf16 operands: each layer's input is split first, one more launch per layer); the head kernels are always exact fp32.

``segment_page`` adds the last stage of ``test_BE_manga.py``: each batch chunk's logits are pasted, where they lie in the plan, into the
page's label map by one more launch (csrc/be_page.hip, ``be_page.compose_page``).

The torchvision backbone is out of scope: the input is its stride-4 feature map.  If the net has one the caller
runs it: ``inf.predict(net.feature_net.backbone(img)["0"])``.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib, be_page, ops, seg_eval
from .infer import FusedVAEInference
from .plan import PlanBuilder, _Plan, _ptr, plan_device

HEAD_WIDTHS = (16, 32, 64)      # MaskNet(in_channel) the head kernels are instantiated for
TILE = (8, 16)                  # feature-map pixels a workgroup of the head kernels owns (csrc/be_infer.h TH x TW)
_HEADS = ("edges", "masks")     # head 0, head 1 of every stacked buffer


def _bn_args(bn):
    return (_ptr(bn.weight), _ptr(bn.bias), _ptr(bn.running_mean), _ptr(bn.running_var))


class FusedBEInference:
    """``features`` / ``predict`` / ``segment`` of a ``networks_BE.ComposeNet`` (its ``aux_convs`` under ``feature_net``) or a
    ``networks_BE_GAN.ComposeNet`` on (n, C, feat_h, feat_w) fp32 feature maps, contiguous or channels_last.

    The plan SNAPSHOTS the model when it is built: weights are folded and packed into plan-owned buffers once, not per call.  After
    the module's parameters or buffers change call ``refresh()``; until then the plan keeps computing with what it was built with.
    Nothing here writes to the module, ``net.training`` is left as found, and the result is eval-mode arithmetic (running statistics)
    whatever the mode.  Inputs of any number of rows run in chunks of ``batch_size``; a short last chunk is padded with zero rows."""

    _run, _capture, _chunks = FusedVAEInference._run, FusedVAEInference._capture, FusedVAEInference._chunks
    _load = staticmethod(FusedVAEInference._load)

    def __init__(self, net, batch_size: int, feat_h: int, feat_w: int, precision: str = "f32", _plan_only: bool = False):
        if precision not in ("f32", "bf16x3"):
            raise ValueError("precision must be 'f32' or 'bf16x3'")
        if batch_size <= 0 or feat_h <= 0 or feat_w <= 0:
            raise ValueError("batch_size, feat_h and feat_w must be positive")
        self.net, self.precision = net, precision
        self.aux = list(net.aux_convs if hasattr(net, "aux_convs") else net.feature_net.aux_convs)
        self.heads = (net.edge_net, net.mask_net)
        self.C = self.aux[0].conv[0].weight.shape[1]
        self.width = self.heads[0].conv1.conv[0].conv[0].weight.shape[1] - 2
        if self.width not in HEAD_WIDTHS:
            raise ValueError(f"FusedBEInference: head width {self.width} is not supported; the head kernels take MaskNet(in_channel) "
                             f"with in_channel in {HEAD_WIDTHS}")
        if self.aux[-1].conv[0].weight.shape[0] != self.width:
            raise ValueError(f"aux_convs ends in {self.aux[-1].conv[0].weight.shape[0]} channels, the heads take {self.width}")
        for head in self.heads:
            for up in (head.conv1, head.conv2):
                if not up.if_add_coord or up.add_coord.if_normalize:
                    raise ValueError("FusedBEInference: the head kernels compute unnormalised coordinate channels (if_normalize=False)")
        self.B, self.h, self.w = int(batch_size), int(feat_h), int(feat_w)
        self.dev = plan_device(net, "FusedBEInference", _plan_only)
        self._bufs: Dict[str, torch.Tensor] = {}
        self._graphs: Dict[str, "torch.cuda.CUDAGraph"] = {}
        self._build()
        if not _plan_only:
            self.refresh()

    # ---- plan construction ------------------------------------------------------------------
    def _build(self):
        B, h, w, C, cw, P = self.B, self.h, self.w, self.C, self.width, _ptr
        lib = _lib.load()
        b = PlanBuilder(self, self.dev, self.precision, side_on=False, wgrad_cus=(0, 0))
        prep, to_nhwc, p_aux, p_up, p_pred, p_seg = (_Plan() for _ in range(6))
        x3 = self.precision == "bf16x3"

        # ---- aux_convs: the folded scale in the weight, the folded shift as the bias ----
        self.x_in = b.buf("x_in", B * C * h * w)                 # the caller's memory order: NCHW, or NHWC as it is
        self.x_nhwc = b.buf("x_nhwc", B * h * w * C)
        to_nhwc.add("vp_nchw_to_nhwc_f32", P(self.x_in), P(self.x_nhwc), B, C, h, w)
        cur = None                                               # (layer 0's input: patched per list below)
        for i, layer in enumerate(self.aux):
            conv, bn = layer.conv[0], layer.conv[1]
            cout, cin, ks = conv.weight.shape[0], conv.weight.shape[1], conv.kernel_size
            wf, shift = b.buf(f"aux{i}.wf", cout, cin, ks, ks), b.buf(f"aux{i}.shift", cout)
            prep.add("vp_be_fold_conv_f32", P(conv.weight), *_bn_args(bn), float(bn.eps), P(wf), P(shift), cout, cin * ks * ks,
                     tag=f"aux{i}.fold")
            out = b.buf(f"aux{i}.y", B * h * w * cout)
            geom = (B, h, w, h, w, cin, cout, ks, 1, ops.ACT_RELU)
            flops = 2.0 * B * h * w * cin * cout * ks * ks
            if x3:
                p0 = b.sbuf(f"aux{i}.p0s", cout * cin * ks * ks)
                prep.add("vp_pack_w_split", P(wf), P(p0), None, cout, cin, ks, tag=f"aux{i}.pack")
                xs = b.sbuf(f"aux{i}.xs", B * h * w * cin)
                p_aux.add("vp_split_f32", P(cur), P(xs), B * h * w * cin, tag=f"aux{i}.split")
                p_aux.add("vp_conv_gather_bf16x3", P(xs), P(p0), P(shift), P(out), *geom, flops=flops, tag=f"aux{i}.fwd")
            else:
                p0 = b.buf(f"aux{i}.p0", cout, ks * ks, cin)
                prep.add("vp_pack_w_f32", P(wf), P(p0), None, cout, cin, ks, tag=f"aux{i}.pack")
                p_aux.add("vp_conv_gather_f32", P(cur), P(p0), P(shift), P(out), *geom, flops=flops, tag=f"aux{i}.fwd")
            cur = out
        self.feat = cur.view(B, h, w, cw)
        # the first layer reads the transposed copy, or -- in the lists for channels_last inputs -- the input where it lies
        p_aux_cl = _Plan()
        p_aux_cl.calls = [list(c) for c in p_aux.calls]
        p_aux_cl.calls[0][2] = list(p_aux.calls[0][2])
        p_aux.calls[0][2][0], p_aux_cl.calls[0][2][0] = P(self.x_nhwc), P(self.x_in)

        # ---- the heads: two Up launches and one predictor launch for both ----
        c1, c2 = cw // 4, cw // 8
        n_up1, n_up2, n_pr = lib.vp_be_up_params_floats(cw, c1), lib.vp_be_up_params_floats(c1, c2), lib.vp_be_predictor_params_floats(c2)
        assert lib.vp_be_infer_supported(cw, c1) and lib.vp_be_infer_supported(c1, c2) and n_pr
        par1, par2, par3 = b.buf("heads.up1.params", 2, n_up1), b.buf("heads.up2.params", 2, n_up2), b.buf("heads.pred.params", 2, n_pr)
        for k, head in enumerate(self.heads):
            for up, par, ci, cm in ((head.conv1, par1, cw, c1), (head.conv2, par2, c1, c2)):
                l1, l2 = up.conv[0].conv, up.conv[1].conv
                if l1[1].eps != l2[1].eps:
                    raise ValueError("the two BatchNorms of an Up block must share eps")
                prep.add("vp_be_up_pack_f32", P(l1[0].weight), *_bn_args(l1[1]), P(l2[0].weight), *_bn_args(l2[1]), float(l1[1].eps),
                         P(par[k]), ci, cm, tag=f"heads.{_HEADS[k]}.pack")
            q = [m.conv[0] for m in head.predictor]
            prep.add("vp_be_predictor_pack_f32", P(q[0].weight), P(q[0].bias), P(q[1].weight), P(q[1].bias), P(q[2].weight), P(q[2].bias),
                     P(par3[k]), c2, tag=f"heads.{_HEADS[k]}.pack")
        H2, W2, H4, W4 = 2 * h, 2 * w, 4 * h, 4 * w
        u1, u2 = b.buf("heads.u1", 2, B, H2, W2, c1), b.buf("heads.u2", 2, B, H4, W4, c2)
        self.logits = b.buf("heads.logits", 2, B, 1, H4, W4)
        self.masks = torch.empty((2, B, 1, H4, W4), dtype=torch.uint8, device=self.dev)
        self._bufs["heads.masks"] = self.masks
        p_up.add("vp_be_up_infer_f32", P(cur), 0, P(par1), P(u1), 2, B, h, w, cw, c1, tag="heads.up1")
        p_up.add("vp_be_up_infer_f32", P(u1), u1[0].numel(), P(par2), P(u2), 2, B, H2, W2, c1, c2, tag="heads.up2")
        pred = (P(u2), u2[0].numel(), P(par3), P(self.logits))
        p_pred.add("vp_be_predictor_infer_f32", *pred, None, 0.0, 2, B, H4, W4, c2, tag="heads.pred")
        self._threshold = 0.5
        p_seg.add("vp_be_predictor_infer_f32", *pred, P(self.masks), self._threshold, 2, B, H4, W4, c2, tag="heads.pred")
        self._seg_args = p_seg.calls[0][2]
        self._prep = prep
        self._n_side_events = 0
        self._plans = {"features": (to_nhwc, p_aux), "predict": (to_nhwc, p_aux, p_up, p_pred), "segment": (to_nhwc, p_aux, p_up, p_seg),
                       "features.cl": (p_aux_cl,), "predict.cl": (p_aux_cl, p_up, p_pred), "segment.cl": (p_aux_cl, p_up, p_seg)}

    # ---- execution ---------------------------------------------------------------------------
    def refresh(self) -> None:
        """Re-read the model: fold every BatchNorm, pack the ``aux_convs`` weights and the heads' parameter blocks.  Runs when the plan
        is built; call it again after the module's parameters or buffers changed.  Graphs captured before are captured again (as
        ``FusedVAEInference.refresh`` does, for the reason given there)."""
        self._prep.run(torch.cuda.current_stream().cuda_stream)
        if self._graphs:
            self._graphs = {}
            self.capture()

    def capture(self, warmup: int = 2):
        """Capture every launch list into one hipGraph each and replay them from then on; the results are bit-identical to the eager
        launches."""
        self._graphs = self._capture(list(self._plans), warmup)
        return self._graphs

    def _feed(self, x: torch.Tensor):
        """validate x; returns (x as it will be copied, the list suffix, the view of the input buffer that takes a chunk)"""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _lib.VaePlayHipError("FusedBEInference: x must be a tensor on the HIP device (no CPU path exists)")
        if x.dtype != torch.float32:
            raise _lib.VaePlayHipError(f"FusedBEInference: x must be fp32, got {x.dtype}")
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.C, self.h, self.w) or x.shape[0] == 0:
            raise _lib.VaePlayHipError(f"FusedBEInference: x has shape {tuple(x.shape)}, this plan takes (n, {self.C}, {self.h}, {self.w})")
        if x.is_contiguous(memory_format=torch.channels_last):
            return x.permute(0, 2, 3, 1), ".cl", self.x_in.view(self.B, self.h, self.w, self.C)
        return x.contiguous(), "", self.x_in.view(self.B, self.C, self.h, self.w)

    def features(self, x: torch.Tensor) -> torch.Tensor:
        """the ``aux_convs`` output (n, width, feat_h, feat_w), channels_last"""
        src, cl, static = self._feed(x)
        n = x.shape[0]
        out = torch.empty((n, self.width, self.h, self.w), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        for i0, m in self._chunks(n):
            self._load(static, src[i0:i0 + m])
            self._run("features" + cl)
            out[i0:i0 + m].copy_(self.feat[:m].permute(0, 3, 1, 2))
        return out

    def _heads_out(self, x, which, with_masks):
        src, cl, static = self._feed(x)
        n = x.shape[0]
        shape = (n, 1, 4 * self.h, 4 * self.w)
        out = {k: x.new_empty(shape) for k in _HEADS}
        if with_masks:
            out.update({k[:-1] + "_mask": torch.empty(shape, dtype=torch.bool, device=x.device) for k in _HEADS})
        for i0, m in self._chunks(n):
            self._load(static, src[i0:i0 + m])
            self._run(which + cl)
            for k, name in enumerate(_HEADS):
                out[name][i0:i0 + m].copy_(self.logits[k, :m])
                if with_masks:
                    out[name[:-1] + "_mask"][i0:i0 + m].copy_(self.masks[k, :m])
        return out

    def predict(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """{"edges", "masks"}: the two heads' logits (n, 1, 4 feat_h, 4 feat_w) of feature maps x, as ``net(x)`` returns them in
        eval mode"""
        return self._heads_out(x, "predict", False)

    def segment(self, x: torch.Tensor, threshold: float = 0.5) -> Dict[str, torch.Tensor]:
        """``predict`` plus "edge_mask" and "mask_mask" (torch.bool) = logits >= threshold (the reference thresholds the raw output,
        test_BE.py:35-39), written by the same predictor launch"""
        threshold = float(threshold)
        if threshold != self._threshold:
            self._seg_args[5] = threshold
            self._threshold = threshold
            if self._graphs:
                self._graphs.update(self._capture(["segment", "segment.cl"]))
        return self._heads_out(x, "segment", True)

    def evaluate(self, x: torch.Tensor, edge_targets: torch.Tensor, mask_targets: torch.Tensor, threshold: float = 0.5, tolerance: int = 0,
                 bce_weight: float = 0.5, smooth: float = 1.0) -> Dict[str, Dict[str, torch.Tensor]]:
        """{"edges": result, "masks": result}, each the ``seg_eval.segmentation_metrics`` result -- per-image loss terms of
        train_BE.py:58-59, confusion counts at ``threshold`` (``segment``'s rule), the boundary match within ``tolerance`` pixels -- of
        the feature maps x against (n, 1, 4 feat_h, 4 feat_w) fp32 targets: every batch chunk runs the ``predict`` launch list and is
        evaluated where its logits lie in the plan, so nothing is copied out.  ``seg_eval.summarize`` reads a result."""
        n = x.shape[0] if isinstance(x, torch.Tensor) and x.dim() == 4 else 0
        for t, what in ((edge_targets, "edge_targets"), (mask_targets, "mask_targets")):
            seg_eval.check_planes(t, what, n or None, (4 * self.h, 4 * self.w))
        src, cl, static = self._feed(x)

        def chunks():
            for i0, m in self._chunks(n):
                self._load(static, src[i0:i0 + m])
                self._run("predict" + cl)
                yield i0, m
        return seg_eval.evaluate_plan(self, n, chunks(), edge_targets, mask_targets, threshold, tolerance, bce_weight, smooth)

    def segment_page(self, x: torch.Tensor, recon_info, boxes, labels, page_hw, original_boxes=None, page_masks=None,
                     variant: str = "result", threshold: float = 0.5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The (H, W, 3) uint8 page label map of ``be_page.compose_page`` for the crops' feature maps x (n, C, feat_h, feat_w), bubble i
        being row i: every batch chunk runs the ``segment`` launch list and is composed straight from the plan's logit planes onto the
        one page, so the per-crop outputs are neither copied out nor held for all n.  ``threshold`` is the page's own (the plan's
        ``segment`` threshold and masks are left alone).  ``n == 0`` gives a white page."""
        H, W = (int(v) for v in page_hw)
        n = int(x.shape[0]) if isinstance(x, torch.Tensor) and x.dim() == 4 else -1
        logit_hw = (4 * self.h, 4 * self.w)
        table = be_page.page_descriptors(recon_info, boxes, labels, (H, W), logit_hw, original_boxes, page_masks is not None, variant)
        if n >= 0 and table.shape[0] != n:
            raise ValueError(f"metadata for {table.shape[0]} bubbles, x has {n} rows")
        if page_masks is not None:
            be_page.check_page_masks(page_masks, table.shape[0], (H, W))
            be_page.require_device(page_masks, "page_masks", self.dev)
        page = be_page.page_buffer(out, (H, W), self.dev)
        if n == 0:
            be_page.launch(None, 0, None, 0, None, 0, None, page, logit_hw, threshold, True)
            return page
        src, cl, static = self._feed(x)
        dtab = table.to(self.dev, non_blocking=True)
        plane = self.logits[0, 0].numel()
        for i0, m in self._chunks(n):
            self._load(static, src[i0:i0 + m])
            self._run("segment" + cl)
            be_page.launch(_ptr(self.logits[0]), plane, _ptr(self.logits[1]), plane, dtab[i0:], m,
                           None if page_masks is None else page_masks[i0:], page, logit_hw, threshold, i0 == 0)
        return page
