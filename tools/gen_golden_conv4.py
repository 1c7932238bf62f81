"""Writes the 4x4 stride-2 fixtures under tests/golden/ from the reference's own modules on the CPU (fp32).
usage: python tools/gen_golden_conv4.py --reference PATH_TO_REFERENCE_CHECKOUT

  stylegan_conv2d_k4s2_instance_relu.npz   models.blocks.Conv2d(8, 16, 4, 2, bn="instance"), the convolution inside myConv2d
                                           (models/network_Style_GAN.py:95-98), on an even (2, 8, 10, 14) and an odd (2, 8, 9, 7) input
  stylegan_convt_k4s2.npz                  bare nn.ConvTranspose2d(16, 8, 4, 2, 1) (:49,116) on (2, 16, 5, 7): holds a bias gradient of order 1
  stylegan_up_16to8.npz                    StyleUp(16, 8) (:45-65) on x (2, 16, 4, 6), skip (2, 8, 8, 12)

Contents (arrays only): param/<key> the state_dict built after torch.manual_seed(seed); x (, skip), gy the randn draws after
torch.manual_seed(seed + 1) in that order; y the output; dx (, dskip) and grad/<key> the gradients of sum(y * gy); seed.  The conv2d
file holds its two cases under the prefixes even/ and odd/ (same parameters).

ReLU margin: every input v of a ReLU that follows a contraction must have min|v| >= 1e-4 * rms(v), so that a mask flip cannot
separate two correct implementations; asserted here, the next seed is taken otherwise.  (The last ReLU of StyleUp.cat_convs sees a
product of its input with positive gates: its zeros are exact in every implementation.)

Run once by a maintainer who has the reference; no test and no GPU job imports this file or needs the reference."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-4


def _run(mod, inputs, relus):
    """forward + backward of mod(*inputs) with a fresh randn gy; returns (arrays, smallest ReLU margin)"""
    seen = []
    hooks = [m.register_forward_hook(lambda _m, i, _o: seen.append(i[0].detach())) for m in relus]
    leaves = [v.clone().requires_grad_(True) for v in inputs]
    mod.zero_grad(set_to_none=True)
    y = mod(*leaves)
    gy = torch.randn(y.shape)
    y.backward(gy)
    for h in hooks:
        h.remove()
    margin = min([(v.abs().min() / v.pow(2).mean().sqrt()).item() for v in seen], default=float("inf"))
    out = {"gy": gy.numpy(), "y": y.detach().numpy()}
    out.update({f"grad/{k}": p.grad.numpy().copy() for k, p in mod.named_parameters()})
    return out, [l.grad.numpy().copy() for l in leaves], margin


def _with_margin(build, what):
    """build(seed) -> (arrays, margin): the first seed from 0 whose ReLU inputs keep the margin"""
    for seed in range(64):
        out, margin = build(seed)
        if margin >= MARGIN:
            out["seed"] = np.array(seed)
            print(f"{what}: seed {seed}, smallest ReLU margin {margin:.2e}")
            return out
        print(f"{what}: seed {seed} rejected (margin {margin:.2e})")
    raise SystemExit(f"{what}: no seed keeps the ReLU margin")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (the directory that holds models/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    sys.path = [p for p in sys.path if os.path.abspath(p or ".") != ROOT]      # `models` must be the reference's package, not this one's
    sys.path.insert(0, os.path.abspath(a.reference))
    from models.blocks import Conv2d
    from models.network_Style_GAN import StyleUp
    for m in ("models.blocks", "models.network_Style_GAN"):
        assert os.path.abspath(sys.modules[m].__file__).startswith(os.path.abspath(a.reference))

    def conv2d(seed):
        torch.manual_seed(seed)
        mod = Conv2d(8, 16, 4, 2, bn="instance")
        out = {f"param/{k}": v.detach().numpy().copy() for k, v in mod.state_dict().items()}
        torch.manual_seed(seed + 1)
        margins = []
        for tag, shape in (("even", (2, 8, 10, 14)), ("odd", (2, 8, 9, 7))):
            x = torch.randn(shape)
            o, (dx,), m = _run(mod, [x], [mod.conv[2]])
            out.update({f"{tag}/{k}": v for k, v in o.items()})
            out[f"{tag}/x"], out[f"{tag}/dx"] = x.numpy(), dx
            margins.append(m)
        return out, min(margins)

    def convt(seed):
        torch.manual_seed(seed)
        mod = torch.nn.ConvTranspose2d(16, 8, 4, 2, 1)
        out = {f"param/{k}": v.detach().numpy().copy() for k, v in mod.state_dict().items()}
        torch.manual_seed(seed + 1)
        x = torch.randn(2, 16, 5, 7)
        o, (dx,), _ = _run(mod, [x], [])
        out.update(o, x=x.numpy(), dx=dx)
        return out, float("inf")

    def up(seed):
        torch.manual_seed(seed)
        mod = StyleUp(16, 8)
        out = {f"param/{k}": v.detach().numpy().copy() for k, v in mod.state_dict().items()}
        torch.manual_seed(seed + 1)
        x, skip = torch.randn(2, 16, 4, 6), torch.randn(2, 8, 8, 12)
        o, (dx, dskip), m = _run(mod, [x, skip], [mod.up_convs[2], mod.cat_convs[0].conv[1]])
        out.update(o, x=x.numpy(), skip=skip.numpy(), dx=dx, dskip=dskip)
        return out, m

    for name, build in (("stylegan_conv2d_k4s2_instance_relu", conv2d), ("stylegan_convt_k4s2", convt), ("stylegan_up_16to8", up)):
        out = _with_margin(build, name)
        path = os.path.join(a.out, name + ".npz")
        np.savez(path, **out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(out)} arrays")


if __name__ == "__main__":
    main()
