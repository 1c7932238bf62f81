"""network_Style_GAN.StyleEncoder and Discriminator on the GPU against the reference-generated fixtures
(tools/gen_golden_stylegan_nets.py) and the fp64 restatement of tests/stylegan_nets_ref.py, in both arithmetic modes.

Outputs against the fixture: 1e-4 in f32, NORTH_STAR_RTOL in bf16x3 (tests/util.rel_err).  Every input and parameter gradient
against the fp64 restatement run on the same parameters, under the whole-network budget of test_gpu_stylegan.test_generator_32_z8:
relative l2 error at most RAW_GRAD_L2[mode], evenly spaced samples within SAMPLE_FACTOR[mode] x that bound in units of the tensor's
RMS.  (No convolution bias sits before an InstanceNorm here -- bn="instance" blocks have none -- so no gradient is mathematically
zero.)  The Discriminator runs with its fused output stage (functional.twin_head) and with the reference's expression; at
image_size 24 the heads see 3 x 3 maps and only the latter exists."""
import pytest
import torch
import torch.nn.functional as F

from tests import stylegan_nets_ref as R
from tests.util import NORTH_STAR_RTOL, RAW_GRAD_L2, SAMPLE_FACTOR, assert_close, record, t

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tol(mode):
    return 1e-4 if mode == "f32" else NORTH_STAR_RTOL


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


def _forward_backward(mod, inputs, consts, grads, mode):
    mod.to(DEV).train()
    mod.zero_grad(set_to_none=True)
    leaves = [v.to(DEV).requires_grad_(True) for v in inputs]
    with _precision(mode):
        outs = mod(*leaves, *consts)
        torch.autograd.backward(list(outs), [g.to(DEV) for g in grads])
        torch.cuda.synchronize()
    return outs, [l.grad for l in leaves]


def _check_gradients(what, mod, dins, ref_dins, ref_grads, names, mode, report):
    bad = []
    for name, got, want in list(zip(names, dins, ref_dins)) + [(k, p.grad, ref_grads[k]) for k, p in mod.named_parameters()]:
        assert got is not None, f"{name}: no gradient"
        if not _budget(f"{what} {name}", got, want, mode, report):
            bad.append(name)
    print("\n".join(report))
    assert not bad, f"{what}: over budget ({mode}): {bad}"


def _fixture_case(which, mod, mode, what, consts=()):
    g = R.fixture(which)
    _, _, n_in, n_g, n_out, n_din = R.FIXTURES[which]
    res = mod.load_state_dict(g["params"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    outs, dins = _forward_backward(mod, [t(g[k]) for k in n_in], consts, [t(g[k]) for k in n_g], mode)
    report = [f"{what} {mode}: " + ", ".join(f"{k} {assert_close(o, t(g[k]), _tol(mode), f'{what} {k} {mode}'):.2e}" for k, o in zip(n_out, outs))
              + " (fixture)"]
    _, ref_dins, ref_grads = R.reference(which)
    _check_gradients(what, mod, dins, ref_dins, ref_grads, n_din, mode, report)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_encoder_16_z8(mode):
    from vae_play_amd import network_Style_GAN as N
    _fixture_case("encoder", N.StyleEncoder(8, 16, max_channels=32), mode, "encoder 16 z8")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_discriminator_16_k3(mode, fused, monkeypatch):
    from vae_play_amd import network_Style_GAN as N
    monkeypatch.setattr(N, "_HEAD_FUSED", fused)
    mod = N.Discriminator(16, 3, max_channels=32)
    g = R.fixture("disc")
    assert mod.uses_fused_head(t(g["x"]), t(g["x_content"])) == fused
    _fixture_case("disc", mod, mode, f"discriminator 16 k3 {'fused' if fused else 'composed'}", consts=(None,))


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_discriminator_24_takes_the_reference_expression(mode):
    """24 -> 12 -> 6 in the trunk, 6 -> 3 -> 2 in the heads: (B, 4) and (B, 4K) in the NCHW order of the reference's reshape"""
    from vae_play_amd import network_Style_GAN as N
    torch.manual_seed(24)
    mod = N.Discriminator(24, 3, max_channels=32)
    x, xc, g_adv, g_aux = torch.randn(2, 3, 24, 24), torch.randn(2, 3, 24, 24), torch.randn(2, 4), torch.randn(2, 12)
    assert not mod.uses_fused_head(x, xc)
    ref_outs, ref_dins, ref_grads = R.run(R.discriminator_forward, mod.state_dict(), [x, xc], [g_adv, g_aux])
    outs, dins = _forward_backward(mod, [x, xc], (None,), [g_adv, g_aux], mode)
    assert tuple(outs[0].shape) == (2, 4) and tuple(outs[1].shape) == (2, 12)
    what = "discriminator 24 k3"
    report = [f"{what} {mode}: " + ", ".join(f"{k} {assert_close(o, r, _tol(mode), f'{what} {k} {mode}'):.2e}"
                                             for k, o, r in zip(("adv", "aux"), outs, ref_outs)) + " (fp64)"]
    _check_gradients(what, mod, dins, ref_dins, ref_grads, ("dx", "dx_content"), mode, report)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_encoder_to_discriminator_chain_and_losses(mode):
    """mu, logvar = E(x); z = reparameterize(mu, logvar); adv, aux = D(x, x_content, y); the KL, adversarial and class losses of
    train_Style_GAN.py:218-219 -- which feeds the softmax's probabilities to F.cross_entropy; reproduced -- on the HIP loss kernels"""
    from vae_play_amd import functional as FH
    from vae_play_amd import network_Style_GAN as N
    ge, gd = R.fixture("encoder"), R.fixture("disc")
    E, D = N.StyleEncoder(8, 16, max_channels=32), N.Discriminator(16, 3, max_channels=32)
    E.load_state_dict(ge["params"], strict=True)
    D.load_state_dict(gd["params"], strict=True)
    E.to(DEV).train()
    D.to(DEV).train()
    x, xc = t(gd["x"]), t(gd["x_content"])
    eps = torch.randn(2, 8, generator=torch.Generator().manual_seed(1))
    y = torch.tensor([0, 2])
    with _precision(mode):
        mu, logvar = E(x.to(DEV))
        z = FH.reparameterize(mu, logvar, eps=eps.to(DEV))
        adv, aux = D(x.to(DEV), xc.to(DEV), None)
        loss = (FH.kl_divergence(mu, logvar).sum() + FH.binary_cross_entropy(adv, torch.ones(2, 1, device=DEV), "mean")
                + FH.cross_entropy(aux, y.to(DEV)))
        loss.backward()
        torch.cuda.synchronize()
    mu64, lv64 = R.encoder_forward({k: v.double() for k, v in ge["params"].items()}, x.double())
    adv64, aux64 = R.discriminator_forward({k: v.double() for k, v in gd["params"].items()}, x.double(), xc.double())
    loss64 = (0.5 * torch.sum(torch.exp(lv64) + mu64 ** 2 - lv64 - 1) + F.binary_cross_entropy(adv64, torch.ones(2, 1, dtype=torch.float64))
              + F.cross_entropy(aux64, y))
    ez = assert_close(z, eps.double() * torch.exp(0.5 * lv64) + mu64, NORTH_STAR_RTOL, f"chain z {mode}")
    el = abs(loss.item() - loss64.item()) / abs(loss64.item())
    print(f"chain {mode}: z {ez:.2e}, loss {loss.item():.6f} against {loss64.item():.6f} (rel {record(f'chain loss {mode}', el):.2e})")
    assert el <= NORTH_STAR_RTOL
    for name, m in (("E", E), ("D", D)):
        for k, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), f"{name}.{k}"
