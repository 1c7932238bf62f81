"""Page compositing for the segmentation heads: the last stage of the reference's deployment path (``test_BE_manga.py``), where the
predictions of every speech-bubble crop of a manga page are pasted back into one page-sized BGR label map -- channels (edge, bubble
type, content), unclaimed pixels white -- which the reference hands to ``cv2.imwrite``.

  * ``variant="result"`` with ``original_boxes``: ``paset_result_on_manga`` as ``main_annotation`` calls it (:63-147, :98-124);
  * ``variant="result"`` with ``page_masks``: the same function without ``original_bubble_boxes`` (:109-113);
  * ``variant="edge"`` (always with ``page_masks``): ``paset_edge_result_on_manga`` (:160-225).

The reference copies the logits to the host and builds several full-page float tensors per bubble; here ONE launch of
csrc/be_page.hip reads the device logits where they lie and writes the page.  The arithmetic is integer and boolean,
so the page equals the reference's byte for byte.  ``page_descriptors`` is the host half: it validates the metadata -- raising
``ValueError`` where the reference would raise or silently wrap -- and builds the int32 table the kernel reads.
"""
from __future__ import annotations

from ctypes import c_void_p
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

DESC_INTS = 16                    # VP_BE_PAGE_DESC_INTS of include/vaeplay_hip.h
KIND_LOGITS, KIND_RECT, KIND_PAGE_MASK, KIND_EDGE_LOGITS = 0, 1, 2, 3
NO_FRAME = 3                      # BUBBLE_TYPES["NoFrame"] (test_BE_manga.py:18-23): the label the heads are not asked about
VARIANTS = ("result", "edge")


def _meta(v, cols: int, what: str, b: Optional[int] = None) -> np.ndarray:
    """metadata as an int64 (rows, cols) array (cols == 0: a vector); a CPU LongTensor, a list or an array"""
    if isinstance(v, torch.Tensor):
        if v.is_floating_point() or v.dtype == torch.bool:
            raise ValueError(f"{what} must hold integers, got {v.dtype}")
        v = v.detach().cpu().numpy()
    a = np.asarray(v)
    if a.size == 0:
        a = np.zeros((0, cols) if cols else (0,), dtype=np.int64)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{what} must hold integers, got {a.dtype}")
    a = a.astype(np.int64)
    if (cols and (a.ndim != 2 or a.shape[1] != cols)) or (not cols and a.ndim != 1):
        raise ValueError(f"{what} must have shape ({'b, ' + str(cols) if cols else 'b'}), got {a.shape}")
    if b is not None and a.shape[0] != b:
        raise ValueError(f"{what} has {a.shape[0]} rows for {b} bubbles")
    return a


def page_descriptors(recon_info, boxes, labels, page_hw: Tuple[int, int], logit_hw: Tuple[int, int], original_boxes=None,
                     has_page_masks: bool = False, variant: str = "result") -> torch.Tensor:
    """Validate one page's metadata and return the (b, 16) int32 CPU table csrc/be_page.hip reads (row layout:
    include/vaeplay_hip.h).  A pure host function.  ``recon_info`` rows are (anchor_x, anchor_y, size), ``boxes`` rows half-open
    (xmin, ymin, xmax, ymax) on the (H, W) page, ``logit_hw`` the size of a logit plane."""
    if variant not in VARIANTS:
        raise ValueError(f"variant must be one of {VARIANTS}, got {variant!r}")
    if variant == "result" and (original_boxes is None) == (not has_page_masks):
        raise ValueError("variant 'result' takes exactly one of original_boxes and page_masks")
    if variant == "edge" and (original_boxes is not None or not has_page_masks):
        raise ValueError("variant 'edge' takes page_masks and no original_boxes")
    H, W = (int(v) for v in page_hw)
    SH, SW = (int(v) for v in logit_hw)
    if H < 1 or W < 1 or H * W > 2 ** 30:
        raise ValueError(f"the page must have 1 .. 2^30 pixels, got {H} x {W}")
    if SH < 1 or SW < 1:
        raise ValueError(f"the logit planes must not be empty, got {SH} x {SW}")
    info = _meta(recon_info, 3, "recon_info")
    b = info.shape[0]
    box, lab = _meta(boxes, 4, "boxes", b), _meta(labels, 0, "labels", b)
    obox = None if original_boxes is None else _meta(original_boxes, 4, "original_boxes", b)
    tab = np.zeros((b, DESC_INTS), dtype=np.int32)
    for i in range(b):
        ax, ay, size = (int(v) for v in info[i])
        xmin, ymin, xmax, ymax = (int(v) for v in box[i])
        label = int(lab[i])
        w, h = xmax - xmin, ymax - ymin
        if w < 1 or h < 1:
            raise ValueError(f"bubble {i}: box {(xmin, ymin, xmax, ymax)} is empty or reversed")
        if xmin < 0 or ymin < 0 or xmax > W or ymax > H:
            raise ValueError(f"bubble {i}: box {(xmin, ymin, xmax, ymax)} leaves the {H} x {W} page")
        if size < 1 or size >= 2 ** 24 or ax < 0 or ay < 0 or ax + w > size or ay + h > size:
            raise ValueError(f"bubble {i}: anchor ({ax}, {ay}) + extent ({w}, {h}) does not fit its {size} x {size} crop square")
        if not 0 <= label <= 255:
            raise ValueError(f"bubble {i}: label {label} is outside 0..255")
        rect = (0, 0, 0, 0)
        if label != NO_FRAME:
            kind = KIND_EDGE_LOGITS if variant == "edge" else KIND_LOGITS
        elif obox is None:
            kind = KIND_PAGE_MASK
            if w < 2 or h < 2:
                raise ValueError(f"bubble {i}: a label-{NO_FRAME} bubble read from its page mask needs a box of at least 2 x 2, got {w} x {h}")
        else:
            kind = KIND_RECT
            oxmin, oymin, oxmax, oymax = (int(v) for v in obox[i])
            rect = (ax + oxmin - xmin, ay + oymin - ymin, ax + oxmax - xmin, ay + oymax - ymin)
            if min(rect) < 0 or max(rect) > size or rect[0] > rect[2] or rect[1] > rect[3]:
                raise ValueError(f"bubble {i}: the original box in crop coordinates {rect} is reversed or leaves [0, {size}]")
        scale = np.array([np.float32(SW) / np.float32(size), np.float32(SH) / np.float32(size)], dtype=np.float32).view(np.int32)
        tab[i] = (ax, ay, scale[0], scale[1], xmin, ymin, xmax, ymax, *rect, label, kind, 0, 0)
    return torch.from_numpy(tab)


def check_logits(t, what: str, b: int) -> Tuple[int, int]:
    """the host-side conditions on a logits tensor (b, 1, SH, SW): fp32 and contiguous; returns (SH, SW)"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be fp32, got {t.dtype}")
    if t.dim() != 4 or t.shape[0] != b or t.shape[1] != 1:
        raise ValueError(f"{what} must have shape ({b}, 1, SH, SW), got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return int(t.shape[2]), int(t.shape[3])


def check_page_masks(page_masks, b: int, page_hw) -> None:
    H, W = page_hw
    if not isinstance(page_masks, torch.Tensor) or page_masks.dtype != torch.uint8:
        raise ValueError("page_masks must be a uint8 tensor (non-zero = set)")
    if tuple(page_masks.shape) != (b, H, W) or not page_masks.is_contiguous():
        raise ValueError(f"page_masks must be contiguous with shape ({b}, {H}, {W}), got {tuple(page_masks.shape)}")


def require_device(t, what: str, dev=None) -> None:
    """a tensor the kernel reads or writes lies on the HIP device (``dev``: on that one)"""
    if not t.is_cuda or (dev is not None and t.device != dev):
        raise _lib.VaePlayHipError(f"compose_page: {what} must be on the HIP device{'' if dev is None else ' of the logits'} (no CPU path exists)")


def page_buffer(out, page_hw, dev) -> torch.Tensor:
    H, W = page_hw
    if out is None:
        return torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor of shape ({H}, {W}, 3)")
    require_device(out, "out", dev)
    return out


def launch(edges_ptr, edge_stride, masks_ptr, mask_stride, table, m, page_masks, page, logit_hw, threshold, init_white) -> None:
    """one vp_be_compose_page_u8 launch on the current stream: ``m`` bubbles whose descriptor rows start at ``table``"""
    ptr = lambda t: None if t is None else c_void_p(t.data_ptr())      # noqa: E731
    _lib.call("vp_be_compose_page_u8", edges_ptr, edge_stride, masks_ptr, mask_stride, ptr(table), m, ptr(page_masks), ptr(page),
              page.shape[0], page.shape[1], logit_hw[0], logit_hw[1], float(threshold), int(init_white),
              c_void_p(torch.cuda.current_stream().cuda_stream))


def compose_page(edges, masks, recon_info, boxes, labels, page_hw: Sequence[int], original_boxes=None, page_masks=None,
                 variant: str = "result", threshold: float = 0.5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (H, W, 3) uint8 label map of one page on the device: bubble ``i``'s logits ``edges[i]`` / ``masks[i]`` (b, 1, S, S fp32,
    on the device; ``masks`` may be None for ``variant="edge"``) resized to its ``size`` x ``size`` crop square with torch's nearest
    rule, cut at its anchor and pasted at its box, in order: the first bubble with an edge or content bit at a pixel owns it.
    Metadata may be CPU LongTensors, as the reference's loaders return them, or lists; it is validated on the host
    (``page_descriptors``) and uploaded in one copy.  ``b == 0`` gives a white page."""
    H, W = (int(v) for v in page_hw)
    if edges is None:
        raise ValueError("edges must be a tensor")
    b = int(edges.shape[0]) if isinstance(edges, torch.Tensor) and edges.dim() > 0 else 0
    logit_hw = check_logits(edges, "edges", b)
    if masks is None:
        if variant != "edge":
            raise ValueError("masks may be None only for variant 'edge'")
    elif check_logits(masks, "masks", b) != logit_hw:
        raise ValueError(f"edges and masks differ in shape: {tuple(edges.shape)} and {tuple(masks.shape)}")
    if b == 0:
        logit_hw = (max(logit_hw[0], 1), max(logit_hw[1], 1))
    table = page_descriptors(recon_info, boxes, labels, (H, W), logit_hw, original_boxes, page_masks is not None, variant)
    if page_masks is not None:
        check_page_masks(page_masks, b, (H, W))
    require_device(edges, "edges")
    for t, what in ((masks, "masks"), (page_masks, "page_masks")):
        if t is not None:
            require_device(t, what, edges.device)
    page = page_buffer(out, (H, W), edges.device)
    with torch.cuda.device(edges.device):
        dtab = table.to(edges.device, non_blocking=True) if b else None
        plane = logit_hw[0] * logit_hw[1]
        launch(c_void_p(edges.data_ptr()) if b else None, plane, c_void_p(masks.data_ptr()) if b and masks is not None else None, plane,
               dtab, b, page_masks if b else None, page, logit_hw, threshold, True)
    return page
