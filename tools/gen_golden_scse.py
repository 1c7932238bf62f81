"""Writes tests/golden/blocks_scse_c32_r4.npz from the reference's own models.blocks.SCSEBlock on the CPU (fp32).
usage: python tools/gen_golden_scse.py --reference PATH_TO_REFERENCE_CHECKOUT

Contents (arrays only):
  state/<key>   the state_dict of SCSEBlock(32, reduction=4) built after torch.manual_seed(0)
  x             input (2, 32, 5, 7), torch.manual_seed(1) randn
  dy            upstream gradient of the same shape, the next randn of that generator state
  y             the block's output
  dx            gradient of sum(y * dy) with respect to x
  grad/<key>    the same gradient with respect to each of the six parameters

Run once by a maintainer who has the reference; no test and no GPU job imports this file or needs the reference."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (the directory that holds models/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "blocks_scse_c32_r4.npz"))
    a = ap.parse_args()
    sys.path = [p for p in sys.path if os.path.abspath(p or ".") != ROOT]      # `models` must be the reference's package, not this one's
    sys.path.insert(0, os.path.abspath(a.reference))
    from models.blocks import SCSEBlock
    assert os.path.abspath(sys.modules["models.blocks"].__file__).startswith(os.path.abspath(a.reference))

    torch.manual_seed(0)
    blk = SCSEBlock(32, reduction=4)
    out = {f"state/{k}": v.detach().numpy().copy() for k, v in blk.state_dict().items()}
    torch.manual_seed(1)
    x = torch.randn(2, 32, 5, 7, requires_grad=True)
    dy = torch.randn(2, 32, 5, 7)
    y = blk(x)
    y.backward(dy)
    out.update(x=x.detach().numpy(), dy=dy.numpy(), y=y.detach().numpy(), dx=x.grad.numpy())
    out.update({f"grad/{k}": p.grad.numpy() for k, p in blk.named_parameters()})
    np.savez(a.out, **out)
    print(f"wrote {a.out}: {sorted(out)}")


if __name__ == "__main__":
    main()
