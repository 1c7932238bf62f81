"""Evaluation of the segmentation heads (``networks_BE``, ``networks_BE_GAN``, ``networks_BE_font``): per image the loss terms of
``train_BE.py:58-59`` (``0.5 * BCEWithLogits + compute_dice_loss``), the confusion counts at the threshold the deployment path uses
(``segment``: logit >= threshold) and a tolerant boundary match -- a predicted pixel counts as matched when a target pixel lies within
Chebyshev distance ``tolerance`` in the same image, and the other way round -- the usual way to score an edge map.

The reference has no evaluation: it writes PNG overlays for eyeballing.  This is new functionality, not a
port; only the loss arithmetic is the reference's.  One launch pair of csrc/seg_eval.hip reads the logits where they lie:

  * ``segmentation_metrics`` takes any (n, 1, H, W) fp32 device tensors -- validation inside a training loop on the autograd modules'
    outputs;
  * ``FusedBEInference.evaluate`` / ``FusedFontInference.evaluate`` run their ``predict`` launch list per batch chunk and evaluate both
    heads straight from the plan's logit planes (``evaluate_plan`` below);
  * ``summarize`` turns a result into the figures a validation log prints: pure host code.
"""
from __future__ import annotations

import math
from ctypes import c_void_p
from typing import Dict

import torch

from . import _lib

MAX_TOLERANCE = 4                 # SE_MAXTOL of csrc/seg_eval.hip
MAX_PIXELS = 2 ** 24
SUMS = ("bce", "pt", "p", "t")
TERMS = ("bce", "dice", "loss")
COUNTS = ("pred", "target", "both", "matched_pred", "matched_target", "nonfinite")
FIGURES = ("loss", "bce", "dice", "iou", "precision", "recall", "f1", "boundary_precision", "boundary_recall", "boundary_f")


def check_planes(t, what: str, n=None, hw=None):
    """the host-side conditions on (n, 1, H, W) planes: an fp32 contiguous tensor of 1 .. 2^24 pixels a plane; returns (n, H, W)"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be fp32, got {t.dtype}")
    if t.dim() != 4 or t.shape[1] != 1 or t.shape[0] < 1 or t.shape[2] < 1 or t.shape[3] < 1:
        raise ValueError(f"{what} must have shape (n, 1, H, W) with n, H, W >= 1, got {tuple(t.shape)}")
    if (n is not None and t.shape[0] != n) or (hw is not None and tuple(t.shape[2:]) != tuple(hw)):
        raise ValueError(f"{what} has shape {tuple(t.shape)}, expected ({'n' if n is None else n}, 1, {hw[0]}, {hw[1]})")
    if t.shape[2] * t.shape[3] > MAX_PIXELS:
        raise ValueError(f"{what}: a plane may hold at most 2^24 pixels, got {t.shape[2]} x {t.shape[3]}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return int(t.shape[0]), int(t.shape[2]), int(t.shape[3])


def check_settings(threshold, tolerance, target_threshold=0.5) -> int:
    if isinstance(tolerance, bool) or not isinstance(tolerance, int) or not 0 <= tolerance <= MAX_TOLERANCE:
        raise ValueError(f"tolerance must be an integer in 0..{MAX_TOLERANCE}, got {tolerance!r}")
    for v, what in ((threshold, "threshold"), (target_threshold, "target_threshold")):
        if not math.isfinite(float(v)):
            raise ValueError(f"{what} must be finite, got {v!r}")
    return tolerance


def check_inputs(logits, targets, threshold=0.5, tolerance=0, target_threshold=0.5):
    """everything ``segmentation_metrics`` can refuse on the host (``ValueError``); returns (n, H, W).  Needs no GPU."""
    n, H, W = check_planes(logits, "logits")
    check_planes(targets, "targets", n, (H, W))
    if logits.device != targets.device:
        raise ValueError(f"logits are on {logits.device}, targets on {targets.device}")
    check_settings(threshold, tolerance, target_threshold)
    return n, H, W


def _new_result(n: int, dev) -> Dict[str, torch.Tensor]:
    return {"sums": torch.empty((n, 4), dtype=torch.float32, device=dev), "terms": torch.empty((n, 3), dtype=torch.float32, device=dev),
            "counts": torch.empty((n, 6), dtype=torch.int32, device=dev)}


def _launch(logits_ptr: int, logit_stride: int, targets_ptr: int, target_stride: int, out, heads, B, H, W, threshold, target_threshold,
            bce_weight, smooth, tolerance, ws) -> None:
    """one vp_seg_eval_f32 call on the current stream; ``out`` holds [heads][B][k] tensors"""
    _lib.call("vp_seg_eval_f32", c_void_p(logits_ptr), logit_stride, c_void_p(targets_ptr), target_stride, c_void_p(out["sums"].data_ptr()),
              c_void_p(out["terms"].data_ptr()), c_void_p(out["counts"].data_ptr()), heads, B, H, W, float(threshold),
              float(target_threshold), float(bce_weight), float(smooth), tolerance, c_void_p(ws.data_ptr()), ws.numel() * 8,
              c_void_p(torch.cuda.current_stream().cuda_stream))


def _workspace(heads, B, H, W, tolerance, dev) -> torch.Tensor:
    nbytes = _lib.load().vp_seg_eval_workspace_bytes(heads, B, H, W, tolerance)
    return torch.empty(max(1, (nbytes + 7) // 8), dtype=torch.float64, device=dev)


def segmentation_metrics(logits: torch.Tensor, targets: torch.Tensor, threshold: float = 0.5, tolerance: int = 0,
                         bce_weight: float = 0.5, smooth: float = 1.0, target_threshold: float = 0.5) -> Dict[str, torch.Tensor]:
    """Per image of (n, 1, H, W) fp32 device tensors, on the device and without a host synchronisation:

      * "sums" (n, 4) fp32: sum bce, sum p t, sum p, sum t with p = sigmoid(logit) -- what ``ops.be_loss_fwd`` keeps per sample;
      * "terms" (n, 3) fp32: sum bce / (H W), the dice score (2 sum p t + smooth) / (sum p + sum t + smooth), and the per-image loss
        bce_weight * sum bce / (H W) + 1 - dice, whose mean over the images is ``be_loss(logits, targets, bce_weight, smooth)``;
      * "counts" (n, 6) int32: |P|, |T|, |P & T|, matched_pred, matched_target, nonfinite, with P = (logit >= threshold) (a NaN is not
        predicted), T = (target >= target_threshold), matched_pred the pixels of P with a pixel of T within Chebyshev distance
        ``tolerance`` (0..4) inside the same image, matched_target the mirror image, nonfinite the NaN or +-inf logits.

    Results are bit-reproducible from run to run."""
    n, H, W = check_inputs(logits, targets, threshold, tolerance, target_threshold)
    if not logits.is_cuda:
        raise _lib.VaePlayHipError("segmentation_metrics: logits and targets must be on the HIP device (no CPU path exists)")
    with torch.cuda.device(logits.device):
        out = _new_result(n, logits.device)
        ws = _workspace(1, n, H, W, tolerance, logits.device)
        _launch(logits.data_ptr(), 0, targets.data_ptr(), 0, out, 1, n, H, W, threshold, target_threshold, bce_weight, smooth, tolerance, ws)
    return out


def evaluate_plan(plan, n: int, chunks, edge_targets, mask_targets, threshold, tolerance, bce_weight, smooth):
    """``evaluate`` of the fused plans.  ``plan.logits`` is (2, B, 1, H, W), head 0 = edges; ``chunks`` yields (i0, m) AFTER running the
    plan's ``predict`` list on rows i0 .. i0 + m.  Each chunk is one vp_seg_eval_f32 call over both heads of the plan's logit planes --
    only its m live rows, never the zero padding of a short last chunk -- with the caller's targets read in place at row i0.  (Two
    calls of one head each when ``mask_targets`` does not lie at least m planes above ``edge_targets`` in memory: the entry's head
    stride is unsigned.)"""
    B, H, W = plan.logits.shape[1], plan.logits.shape[3], plan.logits.shape[4]
    targets = (edge_targets, mask_targets)
    for t, what in zip(targets, ("edge_targets", "mask_targets")):
        check_planes(t, what, n, (H, W))
        if t.device != plan.logits.device:
            raise ValueError(f"{what} is on {t.device}, the plan on {plan.logits.device}")
    check_settings(threshold, tolerance)
    dev, plane = plan.logits.device, H * W
    out = [_new_result(n, dev) for _ in targets]
    stage = {k: v.new_empty((2, B) + v.shape[1:]) for k, v in out[0].items()}
    ws = _workspace(2, B, H, W, tolerance, dev)
    settings = (threshold, 0.5, bce_weight, smooth, tolerance, ws)
    for i0, m in chunks:
        at = [t.data_ptr() + 4 * i0 * plane for t in targets]
        apart = (at[1] - at[0]) // 4
        part = {k: v.view(-1)[:2 * m * v.shape[2]].view(2, m, v.shape[2]) for k, v in stage.items()}
        if apart >= m * plane:
            _launch(plan.logits.data_ptr(), B * plane, at[0], apart, part, 2, m, H, W, *settings)
        else:
            for k in range(2):
                _launch(plan.logits[k].data_ptr(), 0, at[k], 0, {name: v[k] for name, v in part.items()}, 1, m, H, W, *settings)
        for k in range(2):
            for name, v in part.items():
                out[k][name][i0:i0 + m].copy_(v[k])
    return {"edges": out[0], "masks": out[1]}


def _ratio(num, den):
    """num / den element by element in float64; 1.0 where den == 0: there was nothing to get wrong"""
    num, den = num.double(), den.double()
    return torch.where(den == 0, torch.ones_like(num), num / torch.where(den == 0, torch.ones_like(den), den))


def _harmonic(a, b):
    """the harmonic mean, 0 for (0, 0)"""
    s = a + b
    return torch.where(s == 0, torch.zeros_like(s), 2 * a * b / torch.where(s == 0, torch.ones_like(s), s))


def _figures(sums, terms, counts, smooth, pooled: bool):
    """the ten figures from (k, 4) sums, (k, 3) terms, (k, 6) counts in float64: per row, or (pooled) from the column totals"""
    bce, dice, loss = terms[:, 0], terms[:, 1], terms[:, 2]
    if pooled:
        s, counts = sums.sum(0, keepdim=True), counts.sum(0, keepdim=True)
        # equal planes: the pooled bce is the mean of the rows'; the loss is linear in bce and dice
        pooled_dice = (2 * s[:, 1] + smooth) / (s[:, 2] + s[:, 3] + smooth)
        bce, loss, dice = bce.mean(0, keepdim=True), (loss + dice).mean(0, keepdim=True) - pooled_dice, pooled_dice
    P, T, PT, mp, mt = (counts[:, k] for k in range(5))
    precision, recall = _ratio(PT, P), _ratio(PT, T)
    bprecision, brecall = _ratio(mp, P), _ratio(mt, T)
    return {"loss": loss, "bce": bce, "dice": dice, "iou": _ratio(PT, P + T - PT), "precision": precision, "recall": recall,
            "f1": _harmonic(precision, recall), "boundary_precision": bprecision, "boundary_recall": brecall,
            "boundary_f": _harmonic(bprecision, brecall)}


def summarize(result, smooth: float = 1.0) -> Dict[str, Dict[str, float]]:
    """{figure: {"micro": ..., "macro": ...}} in float64 for the figures "loss", "bce", "dice", "iou", "precision", "recall", "f1",
    "boundary_precision", "boundary_recall", "boundary_f" of a ``segmentation_metrics`` / ``evaluate`` result (one head).  Pure host
    code: the three tensors are copied to the host once.

    macro: the figure per image, averaged.  micro: the figure of the summed counts and sums (the dice score of the pooled sums with
    ``smooth``, which should be the value the result was computed with; the loss with that dice score).  A ratio whose denominator is
    zero is 1.0 -- there was nothing to get wrong -- and the harmonic mean of 0 and 0 is 0."""
    sums, terms, counts = (torch.as_tensor(result[k]).detach().cpu().double() for k in ("sums", "terms", "counts"))
    if sums.dim() != 2 or sums.shape[1] != 4 or terms.shape != (sums.shape[0], 3) or counts.shape != (sums.shape[0], 6) or not sums.shape[0]:
        raise ValueError("result must hold 'sums' (n, 4), 'terms' (n, 3) and 'counts' (n, 6) with n >= 1")
    macro, micro = _figures(sums, terms, counts, float(smooth), False), _figures(sums, terms, counts, float(smooth), True)
    return {k: {"micro": float(micro[k][0]), "macro": float(macro[k].mean())} for k in FIGURES}
