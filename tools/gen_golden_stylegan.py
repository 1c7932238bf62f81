"""Writes the Style-GAN generator fixtures under tests/golden/ from the reference's own modules on the CPU (fp32).
usage: python tools/gen_golden_stylegan.py --reference PATH_TO_REFERENCE_CHECKOUT

  stylegan_myconv2d.npz   models.network_Style_GAN.myConv2d (:72-79), two cases under the prefixes
      in4/     myConv2d(8, 16, 4, 2, bn="instance") on an even (2, 8, 10, 14) and an odd (2, 8, 9, 7) input (sub-prefixes even/, odd/,
               same parameters), labels [0.25, 1.0]
      plain/   myConv2d(4, 32, 3, 1, activate=None) on (2, 4, 6, 5), labels [0, 1] as int64
    Contents: param/<key> the state_dict built after torch.manual_seed(seed); x, gy the randn draws after torch.manual_seed(seed + 1)
    in that order; label; y; dx and grad/<key> the gradients of sum(y * gy); seed.
    ReLU margin as in tools/gen_golden_conv4.py: every ReLU input v keeps min|v| >= 1e-4 * rms(v), else the next seed is taken.

  stylegan_generator_32_z8.npz (+ stylegan_generator_32_z8_p<i>.npz)   Generator(32, 8) (:81-180), batch 2, labels [0, 1]
    The 7.75 M parameters are not stored.  The main file holds seed; keys and shapes (ordered names; shapes zero-padded to 4 dims);
    x, style, labels, gy (x, style, gy the randn draws after torch.manual_seed(seed + 1) in that order); y, dx, dstyle; init_sums and
    grad_sums [81][2], the fp64 (sum, sum of squares) of every parameter's initial value and gradient.  The shard files hold
    param/<key> and grad/<key> in full for every parameter of at most 40 000 elements, cut so that no file exceeds 900 KB of data.
    Seed condition: the reference in fp32 and the same modules after .double() agree within one tenth of the f32 tolerances of the
    tests (1e-4 for y, 3e-4 for every gradient, relative to the tensor's max; the three up{1,2,3}.up_convs.0.bias gradients are
    mathematically zero because InstanceNorm follows, and are held to max|db| <= 1e-4 * max|dW| of the same layer instead).  No
    ReLU margin is attainable at this size.

Run once by a maintainer who has the reference; no test and no GPU job imports this file or needs the reference."""
import argparse
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-4
SMALL = 40000
SHARD_BYTES = 900 * 1000
TOL_Y, TOL_G = 1e-4, 3e-4
ZERO_BIAS = tuple(f"up{i}.up_convs.0.bias" for i in (1, 2, 3))
ZERO_TOL = 1e-4


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _run(mod, inputs, consts, relus):
    """forward + backward of mod(*inputs, *consts) with a fresh randn gy; returns (arrays, input gradients, smallest ReLU margin)"""
    seen = []
    hooks = [m.register_forward_hook(lambda _m, i, _o: seen.append(i[0].detach())) for m in relus]
    leaves = [v.clone().requires_grad_(True) for v in inputs]
    mod.zero_grad(set_to_none=True)
    y = mod(*leaves, *consts)
    gy = torch.randn(y.shape)
    y.backward(gy)
    for h in hooks:
        h.remove()
    margin = min([(v.abs().min() / v.pow(2).mean().sqrt()).item() for v in seen], default=float("inf"))
    out = {"gy": gy.numpy(), "y": y.detach().numpy()}
    out.update({f"grad/{k}": p.grad.numpy().copy() for k, p in mod.named_parameters()})
    return out, [l.grad.numpy().copy() for l in leaves], margin


def _with_margin(build, what):
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
    from models.network_Style_GAN import Generator, myConv2d
    for m in ("models.blocks", "models.network_Style_GAN"):
        assert os.path.abspath(sys.modules[m].__file__).startswith(os.path.abspath(a.reference))

    def in4(seed):
        torch.manual_seed(seed)
        mod = myConv2d(8, 16, 4, 2, bn="instance")
        out = {f"param/{k}": v.detach().numpy().copy() for k, v in mod.state_dict().items()}
        label = torch.tensor([0.25, 1.0])
        out["label"] = label.numpy()
        torch.manual_seed(seed + 1)
        margins = []
        for tag, shape in (("even", (2, 8, 10, 14)), ("odd", (2, 8, 9, 7))):
            x = torch.randn(shape)
            o, (dx,), m = _run(mod, [x], [label.reshape(2, 1, 1, 1)], [mod.conv_1.conv[2], mod.conv_2.conv[2]])
            out.update({f"{tag}/{k}": v for k, v in o.items()})
            out[f"{tag}/x"], out[f"{tag}/dx"] = x.numpy(), dx
            margins.append(m)
        return out, min(margins)

    def plain(seed):
        torch.manual_seed(seed)
        mod = myConv2d(4, 32, 3, 1, activate=None)
        out = {f"param/{k}": v.detach().numpy().copy() for k, v in mod.state_dict().items()}
        label = torch.tensor([0, 1], dtype=torch.int64)
        torch.manual_seed(seed + 1)
        x = torch.randn(2, 4, 6, 5)
        o, (dx,), _ = _run(mod, [x], [label.reshape(2, 1, 1, 1)], [])
        out.update(o, x=x.numpy(), dx=dx, label=label.numpy())
        return out, float("inf")

    both = {}
    for prefix, build in (("in4", in4), ("plain", plain)):
        both.update({f"{prefix}/{k}": v for k, v in _with_margin(build, f"stylegan_myconv2d {prefix}").items()})
    path = os.path.join(a.out, "stylegan_myconv2d.npz")
    np.savez(path, **both)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(both)} arrays")

    def generator(seed):
        torch.manual_seed(seed)
        mod = Generator(32, 8)
        init = {k: v.detach().clone() for k, v in mod.named_parameters()}
        labels = torch.tensor([0, 1], dtype=torch.int64)
        torch.manual_seed(seed + 1)
        x, style = torch.randn(2, 3, 32, 32), torch.randn(2, 8)
        o, (dx, dstyle), _ = _run(mod, [x, style], [labels], [])
        gy = torch.from_numpy(o["gy"])
        mod64 = copy.deepcopy(mod).double()
        mod64.zero_grad(set_to_none=True)
        x64, s64 = x.double().requires_grad_(True), style.double().requires_grad_(True)
        y64 = mod64(x64, s64, labels)
        y64.backward(gy.double())
        worst, where = _rel(torch.from_numpy(o["y"]), y64) / TOL_Y, "y"
        checks = [("dx", torch.from_numpy(dx), x64.grad), ("dstyle", torch.from_numpy(dstyle), s64.grad)]
        checks += [(k, torch.from_numpy(o[f"grad/{k}"]), p.grad) for k, p in mod64.named_parameters()]
        for k, g32, g64 in checks:
            if k in ZERO_BIAS:        # mathematically zero (InstanceNorm follows): rounding noise, held against the layer's weight gradient
                e = g32.abs().max().item() / (ZERO_TOL * np.abs(o[f"grad/{k[:-4]}weight"]).max())
            else:
                e = _rel(g32, g64) / TOL_G
            if e > worst:
                worst, where = e, k
        print(f"stylegan_generator_32_z8: seed {seed}: fp32 against fp64 worst {worst:.3f} of the f32 tolerance at {where}")
        if worst > 0.1:
            return None
        keys = list(init)
        shapes = np.zeros((len(keys), 4), np.int64)
        for i, k in enumerate(keys):
            shapes[i, :init[k].dim()] = init[k].shape
        sums = lambda t: [t.double().sum().item(), t.double().pow(2).sum().item()]
        main_file = {"seed": np.array(seed), "keys": np.array(keys), "shapes": shapes, "x": x.numpy(), "style": style.numpy(),
                     "labels": labels.numpy(), "gy": o["gy"], "y": o["y"], "dx": dx, "dstyle": dstyle,
                     "init_sums": np.array([sums(init[k]) for k in keys]),
                     "grad_sums": np.array([sums(torch.from_numpy(o[f"grad/{k}"])) for k in keys])}
        full = {}
        for k in keys:
            if init[k].numel() <= SMALL:
                full[f"param/{k}"] = init[k].numpy()
                full[f"grad/{k}"] = o[f"grad/{k}"]
        return main_file, full

    for seed in range(64):
        r = generator(seed)
        if r is not None:
            break
    else:
        raise SystemExit("stylegan_generator_32_z8: no seed meets the fp32 / fp64 condition")
    main_file, full = r
    shards, size = [{}], 0
    for k, v in full.items():
        if size + v.nbytes > SHARD_BYTES:
            shards.append({})
            size = 0
        shards[-1][k] = v
        size += v.nbytes
    n_small = sum(1 for k in full if k.startswith("param/"))
    print(f"stylegan_generator_32_z8: {n_small} small tensors, {sum(v.size for k, v in full.items() if k.startswith('param/'))} floats")
    for name, arrays in [("stylegan_generator_32_z8", main_file)] + [(f"stylegan_generator_32_z8_p{i}", s) for i, s in enumerate(shards)]:
        path = os.path.join(a.out, name + ".npz")
        np.savez(path, **arrays)
        print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(arrays)} arrays")


if __name__ == "__main__":
    main()
