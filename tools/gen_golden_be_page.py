"""Writes the page-compositing fixtures under tests/golden/ from the reference's own paste functions on the CPU.
usage: python tools/gen_golden_be_page.py --reference PATH_TO_REFERENCE_CHECKOUT

  be_page_annot.npz   test_BE_manga.paset_result_on_manga with original_bubble_boxes (what main_annotation runs)
  be_page_mask.npz    test_BE_manga.paset_result_on_manga without them (label-3 bubbles read from their page masks)
  be_page_edge.npz    test_BE_manga.paset_edge_result_on_manga
  Each: n (number of pages) and per page k the arrays p<k>/edges, p<k>/masks (b, 1, S, S) fp32, p<k>/recon_info (b, 3), p<k>/boxes (b, 4),
  p<k>/labels (b,), p<k>/page_hw (2,), p<k>/original_boxes (b, 4) or p<k>/page_masks (b, H, W) uint8, and p<k>/page (H, W, 3) uint8:
  the array the reference handed to cv2.imwrite.  Pages are seeded and synthetic: at most 96 x 96, at most 6 bubbles, S in {8, 16, 20};
  some logits equal the threshold 0.5 exactly and one per page is a NaN.  be_page_annot.npz ends with one hand-made 8 x 8 page whose
  first bubble has label 3 and a 1 x 1 crop square.

test_BE_manga imports modules this tool does not need to be real (cv2, torchvision, models.networks_BE, tools.utils, and
scipy.ndimage.measurements where scipy no longer has it): stubs are installed before the import; cv2.imwrite captures its array and
torchvision.transforms.functional.to_tensor is the one function of it the paste functions call.  Nothing of the reference's text is
copied, only its outputs are stored.  The tool also probes the inputs on which ``vae_play_amd.be_page.page_descriptors`` raises and
prints what the reference does with them.

Run once by a maintainer who has the reference; no test and no GPU job imports this file or needs the reference."""
import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (8, 16, 20)
LABELS = (0, 1, 2, 3, 3, 3, 4, 255)
CAPTURED = []


def install_stubs():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    module("cv2", imwrite=lambda path, array: CAPTURED.append(np.array(array, copy=True)) or True)
    to_tensor = lambda img: torch.from_numpy(np.asarray(img, dtype=np.float32).transpose(2, 0, 1) / 255)      # noqa: E731
    tf = module("torchvision.transforms.functional", to_tensor=to_tensor)
    tr = module("torchvision.transforms", functional=tf)
    ut = module("torchvision.utils")
    module("torchvision", transforms=tr, utils=ut)
    module("models.networks_BE", ComposeNet=object)
    module("models", networks_BE=sys.modules["models.networks_BE"])
    module("tools.utils", makedirs=lambda path: os.makedirs(path, exist_ok=True))
    module("tools", utils=sys.modules["tools.utils"])
    try:
        import scipy.ndimage.measurements  # noqa: F401
    except ImportError:
        meas = module("scipy.ndimage.measurements", label=None)
        nd = sys.modules.get("scipy.ndimage") or module("scipy.ndimage")
        nd.measurements = meas
        if "scipy" not in sys.modules:
            module("scipy", ndimage=nd)


def random_page(rng, kind):
    """one synthetic page: the inputs of a paste function as numpy arrays"""
    H, W = int(rng.integers(33, 97)), int(rng.integers(33, 97))
    b, S = int(rng.integers(2, 7)), int(rng.choice(SIZES))
    info, boxes, labels, oboxes = [], [], [], []
    for i in range(b):
        w, h = int(rng.integers(2, min(W, 48) + 1)), int(rng.integers(2, min(H, 48) + 1))
        xmin = int(rng.choice([0, W - w, rng.integers(0, W - w + 1)]))
        ymin = int(rng.choice([0, H - h, rng.integers(0, H - h + 1)]))
        size = max(w, h) + int(rng.choice([0, 0, 1, 5]))
        ax, ay = int(rng.integers(0, size - w + 1)), int(rng.integers(0, size - h + 1))
        info.append((ax, ay, size))
        boxes.append((xmin, ymin, xmin + w, ymin + h))
        labels.append(int(rng.choice(LABELS)))
        # the original box: inside the box, a few pixels from its border (so the 6-pixel ring is clipped), at times empty, at times
        # reaching the border of the crop square outside the box
        ox0, oy0 = xmin + int(rng.integers(0, min(w, 9))), ymin + int(rng.integers(0, min(h, 9)))
        ox1, oy1 = int(rng.integers(ox0, xmin + w + 1)), int(rng.integers(oy0, ymin + h + 1))
        if rng.random() < 0.25:
            ox0, ox1 = xmin - ax, xmin + (size - ax)
        oboxes.append((ox0, oy0, ox1, oy1))
    page = dict(recon_info=np.array(info, dtype=np.int64), boxes=np.array(boxes, dtype=np.int64), labels=np.array(labels, dtype=np.int64),
                page_hw=np.array((H, W), dtype=np.int64))
    for name in ("edges", "masks"):
        v = (0.5 + 0.6 * rng.standard_normal((b, 1, S, S))).astype(np.float32)
        v[rng.random(v.shape) < 0.05] = 0.5
        v[int(rng.integers(0, b)), 0, int(rng.integers(0, S)), int(rng.integers(0, S))] = np.nan
        page[name] = v
    if kind == "annot":
        page["original_boxes"] = np.array(oboxes, dtype=np.int64)
    else:
        pm = np.zeros((b, H, W), dtype=np.uint8)
        for i in range(b):
            for _ in range(int(rng.integers(1, 5))):              # blobs anywhere on the page: inside the box, at its border, outside
                y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
                pm[i, y:y + int(rng.integers(1, 12)), x:x + int(rng.integers(1, 12))] = 1
            xmin, ymin, xmax, ymax = boxes[i]
            pm[i, max(ymin - 3, 0):ymin + 2, xmin:xmin + 4] = 1    # one that straddles the box's top border
        page["page_masks"] = pm
    return page


def size_one_page():
    """an 8 x 8 page with two bubbles: a label-3 bubble with a 1 x 1 crop square, then a label-1 bubble over it"""
    rng = np.random.default_rng(7)
    return dict(recon_info=np.array([(0, 0, 1), (1, 0, 6)]), boxes=np.array([(2, 2, 3, 3), (0, 1, 5, 7)]), labels=np.array([3, 1]),
                page_hw=np.array((8, 8)), original_boxes=np.array([(2, 2, 3, 3), (0, 0, 0, 0)]),
                edges=(0.5 + rng.standard_normal((2, 1, 8, 8))).astype(np.float32),
                masks=(0.5 + rng.standard_normal((2, 1, 8, 8))).astype(np.float32))


def run_reference(ref, kind, page, img_dir):
    from PIL import Image
    H, W = (int(v) for v in page["page_hw"])
    img_path = os.path.join(img_dir, "page.png")
    Image.fromarray(np.zeros((H, W, 3), dtype=np.uint8)).save(img_path)
    preds = {k: torch.from_numpy(page[k].copy()) for k in ("edges", "masks")}      # (the functions threshold their input in place)
    lists = [torch.from_numpy(page[k]) for k in ("recon_info",)]
    pm = torch.from_numpy(page["page_masks"].astype(np.float32))[:, None] if "page_masks" in page else None
    labels, boxes = torch.from_numpy(page["labels"]), torch.from_numpy(page["boxes"])
    del CAPTURED[:]
    if kind == "edge":
        ref.paset_edge_result_on_manga(img_path, lists[0], pm, labels, boxes, preds, img_dir, "out")
    elif kind == "mask":
        ref.paset_result_on_manga(img_path, lists[0], pm, labels, boxes, preds, img_dir, "out")
    else:
        ref.paset_result_on_manga(img_path, lists[0], None, labels, boxes, preds, img_dir, "out",
                                  original_bubble_boxes=torch.from_numpy(page["original_boxes"]))
    assert len(CAPTURED) == 1
    return CAPTURED[0]


def probe(ref, img_dir):
    """what the reference does on the inputs page_descriptors refuses (printed; nothing is stored)"""
    def page(kind, info, box, label, obox=None, hw=(8, 8)):
        p = dict(recon_info=np.array([info]), boxes=np.array([box]), labels=np.array([label]), page_hw=np.array(hw),
                 edges=np.ones((1, 1, 8, 8), dtype=np.float32), masks=np.ones((1, 1, 8, 8), dtype=np.float32))
        if kind == "annot":
            p["original_boxes"] = np.array([obox])
        else:
            p["page_masks"] = np.ones((1, *hw), dtype=np.uint8)
        return kind, p
    cases = {"label 3, original box, size 1": page("annot", (0, 0, 1), (2, 2, 3, 3), 3, (2, 2, 3, 3)),
             "label 3, page mask, box 1 wide": page("mask", (0, 0, 4), (2, 2, 3, 6), 3),
             "label 3, page mask, box 1 high": page("mask", (0, 0, 4), (2, 2, 6, 3), 3),
             "box leaves the page": page("annot", (0, 0, 4), (6, 6, 10, 10), 1, (6, 6, 8, 8)),
             "anchor + extent > size": page("annot", (2, 0, 4), (0, 0, 4, 4), 1, (0, 0, 2, 2)),
             "label 256": page("annot", (0, 0, 4), (0, 0, 4, 4), 256, (0, 0, 2, 2)),
             "label -1": page("annot", (0, 0, 4), (0, 0, 4, 4), -1, (0, 0, 2, 2))}
    for name, (kind, p) in cases.items():
        try:
            out = run_reference(ref, kind, p, img_dir)
            print(f"probe {name}: the reference returns; bytes at the box's first pixel {out[p['boxes'][0][1], p['boxes'][0][0]].tolist()}")
        except Exception as e:      # noqa: BLE001
            print(f"probe {name}: the reference raises {type(e).__name__}: {str(e)[:100]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (the directory that holds test_BE_manga.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--pages", type=int, default=6)
    a = ap.parse_args()
    sys.path = [p for p in sys.path if os.path.abspath(p or ".") != ROOT]      # `models` / `tools` must not be this project's
    install_stubs()
    sys.path.insert(0, os.path.abspath(a.reference))
    import test_BE_manga as ref
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(a.reference))
    with tempfile.TemporaryDirectory() as img_dir:
        for seed, kind in enumerate(("annot", "mask", "edge")):
            rng = np.random.default_rng(1000 + seed)
            pages = [random_page(rng, kind) for _ in range(a.pages)]
            if kind == "annot":                                     # a label-3 bubble whose crop square is one pixel (see probe())
                pages.append(size_one_page())
            arrays = {"n": np.array(len(pages))}
            for k, page in enumerate(pages):
                page["page"] = run_reference(ref, kind, page, img_dir)
                if kind == "edge":
                    del page["masks"]
                arrays.update({f"p{k}/{name}": v for name, v in page.items()})
            path = os.path.join(a.out, f"be_page_{kind}.npz")
            np.savez_compressed(path, **arrays)
            print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(pages)} pages")
        probe(ref, img_dir)


if __name__ == "__main__":
    main()
