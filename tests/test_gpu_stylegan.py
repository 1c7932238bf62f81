"""network_Style_GAN.myConv2d and Generator on the GPU against the reference-generated fixtures (tools/gen_golden_stylegan.py) and
the fp64 restatement of tests/stylegan_ref.py, in both arithmetic modes.

myConv2d: the ``_tols`` of tests/test_gpu_conv4.py -- (1e-4, 3e-4) in f32, NORTH_STAR_RTOL in bf16x3 -- with the fused form
(one stacked convolution + functional.pair_blend) and the composed one (the reference's expression over two Conv2d blocks).

Generator(32, 8): y against the fixture; dx, dstyle and every parameter gradient against the fp64 restatement run on the same
seeded parameters, under the project's whole-network budgets for ReLU-mask flips (tests/util.py): relative l2 error at most
RAW_GRAD_L2[mode], evenly spaced samples within SAMPLE_FACTOR[mode] x that bound in units of the tensor's RMS.  About 450 k values
enter a ReLU and 42 of them lie below 1e-4 of their tensor's RMS at this seed, so a flip is possible and a per-element
tolerance is not.  The three up{1,2,3}.up_convs.0.bias gradients are mathematically zero (InstanceNorm follows) and are held to
max|db| <= 1e-4 * max|dW| of the same layer, as test_fixture_styleup_16to8 does."""
import numpy as np
import pytest
import torch

from tests import stylegan_ref as R
from tests.util import NORTH_STAR_RTOL, RAW_GRAD_L2, SAMPLE_FACTOR, assert_close, load_golden, record, t

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tols(mode):
    return (1e-4, 3e-4) if mode == "f32" else (NORTH_STAR_RTOL, NORTH_STAR_RTOL)


class _precision:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from vae_play_amd import functional as FH
        self.prev = FH.get_conv_precision()
        FH.set_conv_precision(self.mode)

    def __exit__(self, *a):
        from vae_play_amd import functional as FH
        FH.set_conv_precision(self.prev)


def _sub(g, prefix):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


MYCONV = {"in4": (dict(in_channel=8, out_channel=16, kernel_size=4, stride=2, bn="instance"), ("even/", "odd/")),
          "plain": (dict(in_channel=4, out_channel=32, kernel_size=3, stride=1, activate=None), ("",))}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", ["in4", "plain"])
def test_fixture_myconv2d(case, mode, fused, monkeypatch):
    from vae_play_amd import network_Style_GAN as N
    g = _sub(load_golden("stylegan_myconv2d"), case + "/")
    kwargs, tags = MYCONV[case]
    ty, tg = _tols(mode)
    monkeypatch.setattr(N, "_PAIR_FUSED", fused)
    mod = N.myConv2d(**kwargs)
    res = mod.load_state_dict({k: t(v) for k, v in _sub(g, "param/").items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    mod.to(DEV).train()
    label = t(g["label"]).to(DEV).reshape(-1, 1, 1, 1)           # as Generator.encode passes it (int64 in the plain case)
    with _precision(mode):
        for tag in tags:
            c = _sub(g, tag) if tag else g
            mod.zero_grad(set_to_none=True)
            x = t(c["x"]).to(DEV).requires_grad_(True)
            assert mod.uses_fused(x, label) == fused
            y = mod(x, label)
            y.backward(t(c["gy"]).to(DEV))
            torch.cuda.synchronize()
            what = f"{case} {tag}{mode} {'fused' if fused else 'composed'}"
            errs = {"y": assert_close(y, t(c["y"]), ty, f"y {what}"), "dx": assert_close(x.grad, t(c["dx"]), tg, f"dx {what}")}
            for k, p in mod.named_parameters():
                errs[k] = assert_close(p.grad, t(c[f"grad/{k}"]), tg, f"grad {k} {what}")
            print(f"fixture myConv2d {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))


def test_myconv2d_takes_any_per_image_label_and_falls_back_otherwise():
    """(B,), (B, 1, 1, 1), float or int64 give the same bits on the fused path; a per-pixel label runs the reference's expression"""
    from vae_play_amd import network_Style_GAN as N
    torch.manual_seed(3)
    mod = N.myConv2d(8, 16, 4, 2, bn="instance").to(DEV)
    x = torch.randn(2, 8, 10, 6, device=DEV)
    with torch.no_grad():
        y0 = mod(x, torch.tensor([0, 1], device=DEV))
        for lab in (torch.tensor([0.0, 1.0], device=DEV), torch.tensor([0, 1], device=DEV).reshape(2, 1, 1, 1), torch.tensor([0, 1])):
            assert torch.equal(mod(x, lab), y0)
        gate = torch.tensor([0.0, 1.0], device=DEV).reshape(2, 1, 1, 1).expand(2, 1, 5, 3).contiguous()
        assert not mod.uses_fused(x, gate)
        assert_close(mod(x, gate), y0, 1e-5, "per-pixel label (composed) against per-image label (fused)")


def _budget(name, got, ref, mode, report):
    """whole-network gradient budget: relative l2 error and evenly spaced samples in RMS units"""
    got, ref = got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten()
    l2 = ((got - ref).norm() / (ref.norm() + 1e-300)).item()
    step = max(1, ref.numel() // 4096)
    rms = (ref.norm() / ref.numel() ** 0.5).item()
    samp = ((got[::step] - ref[::step]).abs().max() / (rms + 1e-300)).item()
    record(f"{name} rel l2 {mode}", l2)
    record(f"{name} sample/rms {mode}", samp)
    report.append(f"  {name}: rel l2 {l2:.2e}, worst sample / rms {samp:.2e}")
    return l2 <= RAW_GRAD_L2[mode] and samp <= SAMPLE_FACTOR[mode] * RAW_GRAD_L2[mode]


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_generator_32_z8(mode):
    from vae_play_amd import network_Style_GAN as N
    g = R.load_generator_fixture()
    torch.manual_seed(int(g["seed"]))
    gen = N.Generator(32, 8)
    for (k, v), (s, q) in zip(gen.state_dict().items(), g["init_sums"]):
        d = v.double()
        assert abs(d.sum().item() - s) <= 1e-6 * abs(s) and abs(d.pow(2).sum().item() - q) <= 1e-6 * q, \
            f"seeded init of {k} differs from the fixture's: the generator was not built like the reference's"
    ref = R.generator_reference(gen.state_dict(), g)
    gen.to(DEV).train()
    x, style = (t(g[k]).to(DEV).requires_grad_(True) for k in ("x", "style"))
    with _precision(mode):
        y = gen(x, style, t(g["labels"]).to(DEV))
        assert tuple(y.shape) == (2, 3, 32, 32)
        y.backward(t(g["gy"]).to(DEV))
        torch.cuda.synchronize()
    ey = assert_close(y, t(g["y"]), 1e-4 if mode == "f32" else NORTH_STAR_RTOL, f"generator y {mode}")
    report, bad = [f"generator 32 z8 {mode}: y {ey:.2e} (fixture), {record('y against fp64 ' + mode, (y.detach().cpu().double() - ref['y']).abs().max().item()):.2e} abs (fp64)"], []
    for name, got, want in [("dx", x.grad, ref["dx"]), ("dstyle", style.grad, ref["dstyle"])] + \
                           [(k, p.grad, ref[f"grad/{k}"]) for k, p in gen.named_parameters()]:
        assert got is not None, f"{name}: no gradient"
        if name in R.ZERO_BIAS:
            db, dW = got.abs().max().item(), dict(gen.named_parameters())[name[:-4] + "weight"].grad.abs().max().item()
            report.append(f"  {name}: max|db| {db:.2e} beside max|dW| {dW:.2e}")
            ok = db <= 1e-4 * dW
        else:
            ok = _budget(name, got, want, mode, report)
        if not ok:
            bad.append(name)
    print("\n".join(report))
    assert not bad, f"over budget ({mode}): {bad}"
