"""Writes tests/golden/seg_eval.npz: the reference's segmentation training loss (train_BE.py:58) on the seeded inputs of the
segmentation-evaluation tests, from the reference's own ``compute_dice_loss`` on the CPU.
usage: python tools/gen_golden_seg_eval.py --reference PATH_TO_REFERENCE_CHECKOUT

  n (number of cases) and per case k: c<k>/family (0 ring, 1 sparse), c<k>/seed, c<k>/logits, c<k>/targets (B, 1, H, W) fp32,
  c<k>/loss32 and c<k>/loss64 = 0.5 * F.binary_cross_entropy_with_logits(x, t) + compute_dice_loss(x.sigmoid(), t), evaluated in fp32
  and on ``.double()`` inputs.

The reference's tools/ops.py is loaded by path: importing it as a module would pull in tools/utils.py and with it cv2 and skimage,
which this tool does not need, so ``tools.utils`` is a stub with the one name ops.py imports.  Nothing of the reference's text is copied,
only its outputs are stored.  Run once by a maintainer who has the reference; no test and no GPU job imports this file or needs the
reference."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 2, 5, 7), (1, 3, 12, 20))          # (heads, B, H, W): small enough to keep the file under 64 KB
SEEDS = (0, 1)


def load_reference_ops(reference):
    path = os.path.join(os.path.abspath(reference), "tools", "ops.py")
    utils = types.ModuleType("tools.utils")
    utils.angle_between = None
    saved = {k: sys.modules.get(k) for k in ("tools", "tools.utils")}
    sys.modules["tools"], sys.modules["tools.utils"] = types.ModuleType("tools"), utils
    try:
        spec = importlib.util.spec_from_file_location("reference_tools_ops", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (the directory that holds tools/ops.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "seg_eval.npz"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from tests import seg_eval_ref as R
    dice = load_reference_ops(a.reference).compute_dice_loss

    def loss(x, t):
        return 0.5 * F.binary_cross_entropy_with_logits(x, t) + dice(x.sigmoid(), t)

    arrays, k = {}, 0
    for fam, name in enumerate(("ring", "sparse")):
        for shape in SHAPES:
            for seed in SEEDS:
                x, t = R.case(name, shape, seed)
                x, t = x[0], t[0]
                arrays.update({f"c{k}/family": np.array(fam), f"c{k}/seed": np.array(seed), f"c{k}/logits": x.numpy(),
                               f"c{k}/targets": t.numpy(), f"c{k}/loss32": np.array(loss(x, t).item(), dtype=np.float32),
                               f"c{k}/loss64": np.array(loss(x.double(), t.double()).item(), dtype=np.float64)})
                k += 1
    arrays["n"] = np.array(k)
    np.savez_compressed(a.out, **arrays)
    size = os.path.getsize(a.out)
    assert size < 64 * 1024, size
    print(f"wrote {a.out} ({size} bytes): {k} cases")


if __name__ == "__main__":
    main()
