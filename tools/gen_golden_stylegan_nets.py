"""Writes the Style-GAN StyleEncoder and Discriminator fixtures under tests/golden/ from the reference's own modules on the CPU (fp32).
usage: python tools/gen_golden_stylegan_nets.py --reference PATH_TO_REFERENCE_CHECKOUT

  stylegan_encoder_16_z8.npz   models.network_Style_GAN.StyleEncoder(8, 16, max_channels=32) (:12-43), batch 2
      x, g_mu, g_logvar (the randn draws after torch.manual_seed(seed + 1), in that order); mu, logvar; dx; 51 536 parameter floats
  stylegan_disc_16_k3.npz      models.network_Style_GAN.Discriminator(16, 3, max_channels=32) (:201-229), batch 2
      x, x_content, g_adv, g_aux (the randn draws after torch.manual_seed(seed + 1), in that order); adv, aux; dx, dx_content;
      56 964 parameter floats
  Both: seed; keys (ordered names); param/<key> the state_dict built after torch.manual_seed(seed); grad/<key> and the input
  gradients those of sum_i sum(output_i * g_i).  Every tensor is stored in full; a file that would pass 900 KB of data is cut
  into <name>_p<i>.npz shards as tools/gen_golden_stylegan.py does (neither does at these sizes).
  Seed rule, the ReLU margin of tools/gen_golden_conv4.py: every value v entering a ReLU or LeakyReLU keeps
  min|v| >= 1e-4 * rms(v) of its tensor, else the next seed is taken.  The fp32 run is also printed against the same modules after
  .double() (outputs and worst gradient, relative to the tensor's max).

Run once by a maintainer who has the reference; no test and no GPU job imports this file or needs the reference."""
import argparse
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-4
SHARD_BYTES = 900 * 1000


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _backward(mod, inputs, grads):
    """forward + backward of sum_i sum(mod(*inputs)[i] * grads[i]); returns (outputs, input gradients, parameter gradients)"""
    leaves = [v.clone().requires_grad_(True) for v in inputs]
    mod.zero_grad(set_to_none=True)
    outs = mod(*leaves)
    torch.autograd.backward(list(outs), [g.to(o.dtype) for g, o in zip(grads, outs)])
    return [o.detach() for o in outs], [l.grad for l in leaves], {k: p.grad for k, p in mod.named_parameters()}


def _case(seed, build, in_shapes, call):
    """One seed of the protocol: {arrays}, the smallest ReLU margin and the number of values that entered a ReLU / LeakyReLU"""
    torch.manual_seed(seed)
    mod = build()
    out = {f"param/{k}": v.detach().numpy().copy() for k, v in mod.state_dict().items()}
    out["keys"] = np.array(list(mod.state_dict()))
    torch.manual_seed(seed + 1)
    inputs = [torch.randn(s) for s in in_shapes]
    seen = []
    relus = [m for m in mod.modules() if isinstance(m, (torch.nn.ReLU, torch.nn.LeakyReLU))]
    hooks = [m.register_forward_hook(lambda _m, i, _o: seen.append(i[0].detach())) for m in relus]
    with torch.no_grad():
        shapes = [o.shape for o in call(mod)(*inputs)]
    for h in hooks:
        h.remove()
    margin = min((v.abs().min() / v.pow(2).mean().sqrt()).item() for v in seen)
    grads = [torch.randn(s) for s in shapes]               # one gradient per output, in output order, after the inputs
    outs, dins, dparams = _backward(call(mod), inputs, grads)
    o64, d64, p64 = _backward(call(copy.deepcopy(mod).double()), [v.double() for v in inputs], grads)
    e_out = max(_rel(a, b) for a, b in zip(outs, o64))
    e_grad = max([_rel(a, b) for a, b in zip(dins, d64)] + [_rel(dparams[k], p64[k]) for k in dparams])
    out.update({f"grad/{k}": v.numpy().copy() for k, v in dparams.items()})
    return out, inputs, grads, outs, dins, margin, sum(v.numel() for v in seen), e_out, e_grad


class _Call(torch.nn.Module):
    """mod(*inputs, *consts) as a module of the inputs alone (named_parameters / zero_grad pass through to ``mod``)"""

    def __init__(self, mod, consts):
        super().__init__()
        self.mod, self.consts = mod, consts

    def named_parameters(self, *a, **k):
        return self.mod.named_parameters(*a, **k)

    def forward(self, *inputs):
        return self.mod(*inputs, *self.consts)


def _write(out_dir, name, arrays):
    shards, size = [{}], 0
    for k, v in arrays.items():
        v = np.asarray(v)
        if size + v.nbytes > SHARD_BYTES and shards[-1]:
            shards.append({})
            size = 0
        shards[-1][k] = v
        size += v.nbytes
    for i, s in enumerate(shards):
        path = os.path.join(out_dir, name + ("" if i == 0 else f"_p{i - 1}") + ".npz")
        np.savez(path, **s)
        print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(s)} arrays")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (the directory that holds models/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    sys.path = [p for p in sys.path if os.path.abspath(p or ".") != ROOT]      # `models` must be the reference's package, not this one's
    sys.path.insert(0, os.path.abspath(a.reference))
    from models.network_Style_GAN import Discriminator, StyleEncoder
    for m in ("models.blocks", "models.network_Style_GAN"):
        assert os.path.abspath(sys.modules[m].__file__).startswith(os.path.abspath(a.reference))

    cases = (("stylegan_encoder_16_z8", lambda: StyleEncoder(8, 16, max_channels=32), [(2, 3, 16, 16)], (),
              ("x",), ("g_mu", "g_logvar"), ("mu", "logvar"), ("dx",)),
             ("stylegan_disc_16_k3", lambda: Discriminator(16, 3, max_channels=32), [(2, 3, 16, 16), (2, 3, 16, 16)], (None,),
              ("x", "x_content"), ("g_adv", "g_aux"), ("adv", "aux"), ("dx", "dx_content")))
    for name, build, in_shapes, consts, n_in, n_g, n_out, n_din in cases:
        for seed in range(64):
            out, inputs, grads, outs, dins, margin, n_relu, e_out, e_grad = _case(seed, build, in_shapes, lambda m: _Call(m, consts))
            if margin >= MARGIN:
                break
            print(f"{name}: seed {seed} rejected (margin {margin:.2e})")
        else:
            raise SystemExit(f"{name}: no seed keeps the ReLU margin")
        n_par = sum(v.size for k, v in out.items() if k.startswith("param/"))
        print(f"{name}: seed {seed}, smallest margin {margin:.2e} over {n_relu} ReLU / LeakyReLU inputs, {n_par} parameter floats; "
              f"fp32 against fp64: outputs {e_out:.1e}, gradients {e_grad:.1e}")
        out["seed"] = np.array(seed)
        for names, tensors in ((n_in, inputs), (n_g, grads), (n_out, outs), (n_din, dins)):
            out.update({k: v.numpy().copy() for k, v in zip(names, tensors)})
        _write(a.out, name, out)


if __name__ == "__main__":
    main()
