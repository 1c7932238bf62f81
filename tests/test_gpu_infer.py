"""vae_play_amd.infer.FusedVAEInference on the GPU: end-to-end parity against the CPU oracle evaluated in fp64 (eval mode), next to
the existing module path in ``.eval()`` on the same weights, and the properties that need no oracle (row independence, chunking,
reproducible sampling, determinism, graph replay, refresh(), purity).

Models under test have non-trivial eval state: gamma ~ U(0.5, 1.5) and beta ~ N(0, 0.2) from a seeded generator, then three
train-mode forwards on different seeded batches (momentum 0.9 moves the running statistics to the data's), so that a swapped or
mis-indexed scale / shift cannot pass."""
import pytest
import torch

from tests.util import NORTH_STAR_RTOL, record, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
# relative error of the forward outputs per arithmetic mode
FLOOR = {"f32": 4e-6, "bf16x3": 1.4e-5}
SHAPES = [(1, 32, 16, 4), (3, 64, 64, 4), (3, 128, 128, 32)]      # (C, S, z, B)


def _trained_vae(C, S, z, B, seed=0):
    """a VAE with non-trivial BatchNorm state (see the module docstring), left in eval mode"""
    import vae_play_amd as V
    torch.manual_seed(seed)
    vae = V.VAE(S, z, C).to(DEV)
    g = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        for m in vae.modules():
            if hasattr(m, "num_batches_tracked"):
                m.weight.copy_(torch.empty(m.weight.shape).uniform_(0.5, 1.5, generator=g))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
        vae.train()
        V.set_conv_precision("f32")
        for k in range(3):
            xb = torch.rand((B, C, S, S), generator=torch.Generator().manual_seed(200 + k)).to(DEV)
            eb = torch.randn((B, z), generator=torch.Generator().manual_seed(300 + k)).to(DEV)
            vae(xb, eb)
    torch.cuda.synchronize()
    return vae.eval()


def _batch(C, S, z, n, seed=7):
    x = torch.rand((n, C, S, S), generator=torch.Generator().manual_seed(seed))
    eps = torch.randn((n, z), generator=torch.Generator().manual_seed(seed + 1))
    return x, eps


_ORACLE = {}


def _oracle(vae, C, S, z, B):
    """fp64 eval-mode forward of the CPU oracle on the model's state (one evaluation per shape: both precisions share the model)"""
    from oracle import ref_cpu as O
    key = (C, S, z, B)
    if key not in _ORACLE:
        p64 = {k: (v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu().clone()) for k, v in vae.state_dict().items()}
        x, eps = _batch(C, S, z, B)
        with torch.no_grad():
            out = O.vae_forward(p64, x.double(), eps.double(), vae.iter_level, training=False)
            dec = O.decoder_forward(p64, out["z"].float().double(), vae.iter_level, training=False)
        _ORACLE[key] = ({k: out[k] for k in ("mu", "logvar", "z", "x_tilde")}, dec)
    return _ORACLE[key]


@pytest.mark.parametrize("C,S,z,B", SHAPES)
@pytest.mark.parametrize("prec", ("bf16x3", "f32"))
def test_end_to_end_vs_fp64_oracle(prec, C, S, z, B):
    """encode / decode / reconstruct against the fp64 oracle: (a) within NORTH_STAR_RTOL; (b) err_fused <= max(2 err_modules, floor),
    err_modules = the existing module path in eval mode on the same weights and inputs.  The fused path rounds fma(acc, s, t) where
    the module path rounds ((x - mean) rstd) gamma + beta: neither is systematically better, an indexing bug is orders beyond 2x."""
    import vae_play_amd as V
    vae = _trained_vae(C, S, z, B)
    ref, ref_dec = _oracle(vae, C, S, z, B)
    x, eps = _batch(C, S, z, B)
    x, eps = x.to(DEV), eps.to(DEV)
    z_in = ref["z"].float().to(DEV)
    inf = V.FusedVAEInference(vae, B, S, C, precision=prec)
    xt, mu, logvar = inf.reconstruct(x, eps)
    mu_e, logvar_e = inf.encode(x)
    xd = inf.decode(z_in)
    assert torch.equal(mu_e, mu) and torch.equal(logvar_e, logvar), "encode() and reconstruct() disagree on the encoder"
    V.set_conv_precision(prec)
    try:
        with torch.no_grad():
            xt_m, mu_m, logvar_m = vae(x, eps)
            xd_m = vae.decoder(z_in)
    finally:
        V.set_conv_precision("f32")
    torch.cuda.synchronize()
    tag = f"{prec} {S}x{S}x{C} b{B}"
    pairs = (("mu", mu, mu_m, ref["mu"]), ("logvar", logvar, logvar_m, ref["logvar"]), ("x_tilde", xt, xt_m, ref["x_tilde"]),
             ("decode", xd, xd_m, ref_dec))
    fails = []
    for name, got, mod, want in pairs:
        ef, em = rel_err(got, want), rel_err(mod, want)
        record(f"infer fused {tag} {name}", ef)
        record(f"infer modules {tag} {name}", em)
        print(f"{tag} {name}: fused {ef:.3e}  modules {em:.3e}")
        if not ef <= NORTH_STAR_RTOL:
            fails.append(f"{name}: fused {ef:.3e} > {NORTH_STAR_RTOL:.0e}")
        if not ef <= max(2 * em, FLOOR[prec]):
            fails.append(f"{name}: fused {ef:.3e} > max(2 x modules {em:.3e}, floor {FLOOR[prec]:.1e})")
    assert not fails, "; ".join(fails)
    assert vae.training is False


def _state(vae):
    return {k: v.detach().clone() for k, v in vae.state_dict().items()}, {n: m.training for n, m in vae.named_modules()}


@pytest.mark.parametrize("prec", ("bf16x3", "f32"))
def test_properties_without_oracle(prec):
    import vae_play_amd as V
    C, S, z, B = 3, 64, 64, 32
    vae = _trained_vae(C, S, z, B, seed=1)
    before, flags = _state(vae)
    inf = V.FusedVAEInference(vae, B, S, C, precision=prec)
    g = torch.Generator(device=DEV).manual_seed(5)
    zz = torch.randn((70, z), device=DEV, generator=g)
    x, eps = _batch(C, S, z, 40)
    x, eps = x.to(DEV), eps.to(DEV)

    # two calls give the same bits
    full = inf.decode(zz[:B])
    assert torch.equal(inf.decode(zz[:B]), full)
    r1 = inf.reconstruct(x, eps)
    r2 = inf.reconstruct(x, eps)
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))
    # rows are independent: row i of a full batch == the same latent alone in a zero-padded chunk (same kernels, same tiles)
    for i in (0, 13, B - 1):
        assert torch.equal(inf.decode(zz[i:i + 1]), full[i:i + 1]), f"row {i} depends on its batch"
    e_full = inf.encode(x[:B])
    for i in (0, 13, B - 1):
        e1 = inf.encode(x[i:i + 1])
        assert torch.equal(e1[0], e_full[0][i:i + 1]) and torch.equal(e1[1], e_full[1][i:i + 1]), f"row {i} depends on its batch"
    # chunking: 70 latents with batch_size 32 == three chunked calls
    d70 = inf.decode(zz)
    assert d70.shape == (70, C, S, S)
    assert torch.equal(d70, torch.cat([inf.decode(zz[0:32]), inf.decode(zz[32:64]), inf.decode(zz[64:70])]))
    assert torch.equal(r1[0][32:40], inf.reconstruct(x[32:40], eps[32:40])[0])
    # sample(): reproducible for a seeded generator, and the decode of the same draw
    s1 = inf.sample(40, g.manual_seed(9))
    s2 = inf.sample(40, g.manual_seed(9))
    zd = torch.randn((40, z), device=DEV, generator=g.manual_seed(9))
    assert torch.equal(s1, s2) and torch.equal(s1, inf.decode(zd))
    assert not torch.equal(s1, inf.sample(40, g))              # (the generator moved on)
    # reconstruct without eps SAMPLES (eval mode still draws z), reproducibly for a seeded generator
    ra = inf.reconstruct(x, generator=g.manual_seed(3))
    rb = inf.reconstruct(x, eps=torch.randn((40, z), device=DEV, generator=g.manual_seed(3)))
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], r1[1]) and not torch.equal(ra[0], r1[0])
    # the result is eval-mode arithmetic whatever module.training says, and the flag is left alone
    vae.train()
    assert all(torch.equal(a, b) for a, b in zip(inf.reconstruct(x, eps), r1)) and vae.training
    vae.eval()

    # graph replay == eager, bit for bit; inputs are read at call time
    inf.capture()
    assert torch.equal(inf.decode(zz), d70)
    assert all(torch.equal(a, b) for a, b in zip(inf.reconstruct(x, eps), r1))
    e_g = inf.encode(x[:B])
    assert torch.equal(e_g[0], e_full[0]) and torch.equal(e_g[1], e_full[1])

    # nothing above wrote to the module
    after, flags_after = _state(vae)
    assert flags_after == flags
    for k in before:
        assert torch.equal(before[k], after[k]), f"{k} was modified"

    # refresh(): a stale plan keeps the weights it was built with; refresh() picks the change up (eager and replayed)
    w = vae.decoder.conv[1].conv.weight
    bn = vae.decoder.conv[2].bn
    saved_w, saved_rv = w.detach().clone(), bn.running_var.clone()
    with torch.no_grad():
        w.mul_(1.5)
        bn.running_var.mul_(2.0)
    assert torch.equal(inf.decode(zz), d70), "a stale plan must not see the change"
    inf.refresh()
    d_new = inf.decode(zz)
    assert not torch.equal(d_new, d70)
    V.set_conv_precision(prec)
    try:
        with torch.no_grad():
            d_mod = vae.decoder(zz)
    finally:
        V.set_conv_precision("f32")
    assert rel_err(d_new, d_mod) <= 1e-4, "refresh() did not pick up the new weights / running statistics"
    with torch.no_grad():
        w.copy_(saved_w)
        bn.running_var.copy_(saved_rv)
    inf.refresh()
    d_back = inf.decode(zz)
    assert torch.equal(d_back, d70), f"restored weights + refresh(): max |diff| {(d_back - d70).abs().max().item():.3e}"


def test_vaegan_halves():
    """an Encoder / Decoder pair (a VaeGan's halves, one image channel) against the same modules in eval mode"""
    import vae_play_amd as V
    torch.manual_seed(2)
    net = V.VaeGan(32, 16).to(DEV).eval()
    inf = V.FusedVAEInference.from_modules(net.encoder, net.decoder, 8, 32, 1)
    x, eps = _batch(1, 32, 16, 8)
    x, eps = x.to(DEV), eps.to(DEV)
    V.set_conv_precision("bf16x3")
    try:
        with torch.no_grad():
            mu_m, lv_m = net.encoder(x)
            xt_m = net.decoder(V.reparameterize(mu_m, lv_m, eps=eps))
    finally:
        V.set_conv_precision("f32")
    xt, mu, lv = inf.reconstruct(x, eps)
    assert rel_err(mu, mu_m) <= 1e-4 and rel_err(lv, lv_m) <= 1e-4 and rel_err(xt, xt_m) <= 1e-4
    assert inf.sample(3).shape == (3, 1, 32, 32)


def test_error_paths():
    """host-side validation only"""
    import vae_play_amd as V
    from vae_play_amd import _lib
    torch.manual_seed(0)
    vae = V.VAE(32, 16, 1).to(DEV).eval()
    inf = V.FusedVAEInference(vae, 4, 32, 1)
    with pytest.raises(_lib.VaePlayHipError, match="shape"):
        inf.encode(torch.zeros((2, 3, 32, 32), device=DEV))            # channel count
    with pytest.raises(_lib.VaePlayHipError, match="shape"):
        inf.reconstruct(torch.zeros((2, 1, 64, 64), device=DEV))       # image size
    with pytest.raises(_lib.VaePlayHipError, match="shape"):
        inf.decode(torch.zeros((2, 17), device=DEV))
    with pytest.raises(_lib.VaePlayHipError, match="HIP device"):
        inf.encode(torch.zeros((2, 1, 32, 32)))                        # CPU tensor
    with pytest.raises(_lib.VaePlayHipError, match="fp32"):
        inf.decode(torch.zeros((2, 16), device=DEV, dtype=torch.float64))
    with pytest.raises(_lib.VaePlayHipError, match="rows"):
        inf.reconstruct(torch.zeros((2, 1, 32, 32), device=DEV), eps=torch.zeros((3, 16), device=DEV))
    with pytest.raises(ValueError, match="precision"):
        V.FusedVAEInference(vae, 4, 32, 1, precision="f16x2")
    with pytest.raises(ValueError):
        inf.sample(0)
