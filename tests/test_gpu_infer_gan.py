"""vae_play_amd.infer_gan.FusedVAEGANInference on the GPU: end to end against the fp64 oracle in eval mode (oracle/ref_vaegan.py with
``training=False``) next to the drop-in modules in ``.eval()`` on the same weights, and the properties that need no oracle: the
inherited methods are the parent's bit for bit, the new methods agree with each other, rows are independent, nothing writes the
module, graph replay equals the eager launches, ``refresh()`` picks a changed model up.

Models under test have non-trivial eval state (tests/infer_gan_ref.py).  Shapes are iter_level 1, 2 and 3: at level 1 the tap block
follows the stem directly.

Measured on MI355X (relative error in tests.util.rel_err's norm, fused / modules):
see DESIGN.md 14.4 for the table this test records."""
import pytest
import torch

from tests import infer_gan_ref as R
from tests.guarded import same_bits
from tests.util import NORTH_STAR_RTOL, record, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 1.4e-5          # tests/test_gpu_infer.py's floor of the "bf16x3" mode
SHAPES = [(16, 8, 2), (32, 16, 4), (64, 32, 4)]      # (S, z, B)

_CACHE = {}


def _model(S, z, B):
    """(net, x, eps, oracle results), built once per shape and left unchanged"""
    key = (S, z, B)
    if key not in _CACHE:
        net = R.trained_vaegan(S, z, B)
        x, eps = R.batch(S, z, B)
        _CACHE[key] = (net, x, eps, R.oracle_similarity(net, x, eps))
    return _CACHE[key]


@pytest.mark.parametrize("S,z,B", SHAPES)
def test_end_to_end_vs_fp64_oracle(S, z, B):
    """(a) every output within NORTH_STAR_RTOL of the fp64 oracle; (b) err_fused <= max(2 err_modules, FLOOR): the rule of
    tests/test_gpu_infer.py -- the fused path rounds fma(acc, s, t) where the module path rounds ((x - mean) rstd) gamma + beta and
    one folded map where it runs eight layers; neither is systematically better, an indexing bug is orders beyond 2x."""
    import vae_play_amd as V
    net, x, eps, ref = _model(S, z, B)
    x, eps = x.to(DEV), eps.to(DEV)
    inf = V.FusedVAEGANInference(net, B)
    xt, params = inf.forward(x, eps)
    sim = inf.similarity(x, eps)
    dis = inf.discriminate(torch.cat([x, sim["x_tilde"]]))
    mod = R.modules_similarity(net, x, eps)
    torch.cuda.synchronize()
    got = {"x_tilde": xt, "params": params, "features": dis["features"], "logit": dis["logit"], "p": dis["p"],
           "mse": sim["mse"], "nle": sim["nle"], "bce_dis_original": sim["bce_dis_original"], "bce_dis_predicted": sim["bce_dis_predicted"]}
    tag = f"{S}x{S} z{z} b{B}"
    fails = []
    for name, t in got.items():
        want = ref[name].reshape(t.shape)
        ef, em = rel_err(t, want), rel_err(mod[name].reshape(t.shape), want)
        record(f"infer_gan fused {tag} {name}", ef)
        record(f"infer_gan modules {tag} {name}", em)
        print(f"{tag} {name}: fused {ef:.3e}  modules {em:.3e}")
        if not ef <= NORTH_STAR_RTOL:
            fails.append(f"{name}: fused {ef:.3e} > {NORTH_STAR_RTOL:.0e}")
        if not ef <= max(2 * em, FLOOR):
            fails.append(f"{name}: fused {ef:.3e} > max(2 x modules {em:.3e}, floor {FLOOR:.1e})")
    assert not fails, "; ".join(fails)
    assert net.training is False


@pytest.mark.parametrize("S,z,B", SHAPES)
def test_the_methods_agree_with_each_other_and_with_the_parent(S, z, B):
    import vae_play_amd as V
    from vae_play_amd import ops
    net, x, eps, _ = _model(S, z, B)
    x, eps = x.to(DEV), eps.to(DEV)
    inf = V.FusedVAEGANInference(net, B)
    par = V.FusedVAEInference.from_modules(net.encoder, net.decoder, B, S, 1)
    # the inherited methods, before and after the VAE-GAN lists exist
    zz = torch.randn((B, z), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    eps2 = torch.randn((B, 2, z), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    for when in ("before", "after"):
        for a, b in zip(inf.encode(x) + inf.reconstruct(x, eps) + (inf.decode(zz),), par.encode(x) + par.reconstruct(x, eps) + (par.decode(zz),)):
            assert same_bits(a, b), f"{when} enable_gan(): an inherited result differs from the from_modules plan"
        sa, sb = inf.score(x, 2, eps2), par.score(x, 2, eps2)
        assert all(same_bits(sa[k], sb[k]) for k in sb), f"{when} enable_gan(): score differs"
        inf.enable_gan()
    # x_tilde is reconstruct's
    rec = inf.reconstruct(x, eps)
    xt, params = inf.forward(x, eps)
    sim = inf.similarity(x, eps)
    assert same_bits(xt, rec[0]) and same_bits(sim["x_tilde"], rec[0])
    assert same_bits(sim["mu"], rec[1]) and same_bits(sim["logvar"], rec[2])
    assert same_bits(sim["params"], params)
    zs = eps * torch.exp(rec[2] / 2) + rec[1]
    assert rel_err(inf.params(zs), params) <= 1e-5            # (z formed by torch here, by the latent kernel there)
    # similarity's scores are discriminate's, on x and on that x_tilde
    dx, dt = inf.discriminate(x), inf.discriminate(sim["x_tilde"])
    assert same_bits(sim["p_x"], dx["p"]) and same_bits(sim["p_x_tilde"], dt["p"])
    both = inf.discriminate(torch.cat([x, sim["x_tilde"]]))
    assert same_bits(both["p"], torch.cat([dx["p"], dt["p"]])) and same_bits(both["features"], torch.cat([dx["features"], dt["features"]]))
    # ... and its feature distance is the tap kernel's on discriminate's buffers (the tap's fp32 output of (x | x_tilde))
    c = inf._bufs[f"gan.disc{inf.L}.c"].view(2 * B, 64, -1)
    dist = torch.empty(B, device=DEV)
    ops.disc_tap_eval(c, None, None, None, None, B, dist)
    assert same_bits(sim["mse"], dist)
    assert same_bits(both["features"], c.permute(0, 2, 1).reshape(2 * B, -1).contiguous())
    # the log terms are the head's on those scores
    ref = R.loss_terms(x.double(), sim["x_tilde"].double(), both["features"].double(), both["p"].double())
    for k, v in ref.items():
        assert rel_err(sim[k], v) <= 2e-5, k
    kl = -0.5 * torch.sum(-sim["logvar"].double().exp() - sim["mu"].double() ** 2 + sim["logvar"].double() + 1, 1)
    assert rel_err(sim["kl"], kl) <= 2e-5


def test_rows_purity_replay_refresh():
    import vae_play_amd as V
    S, z, B = 16, 8, 2
    net = R.trained_vaegan(S, z, B, seed=1)
    before, flags = R.state(net)
    inf = V.FusedVAEGANInference(net, B)
    x, eps = R.batch(S, z, 3, seed=11)
    x, eps = x.to(DEV), eps.to(DEV)

    def run(which, xs, es, plan=inf):
        if which == "params":
            return {"params": plan.params(es)}
        if which == "forward":
            return dict(zip(("x_tilde", "params"), plan.forward(xs, es)))
        return plan.discriminate(xs) if which == "discriminate" else plan.similarity(xs, es)
    zlat = torch.randn((3, z), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    eager = {}
    for which in ("params", "forward", "discriminate", "similarity"):
        es = zlat if which == "params" else eps
        full = eager[which] = run(which, x, es)
        again = run(which, x, es)
        assert all(same_bits(full[k], again[k]) for k in full), f"{which}: two calls differ"
        for i in range(3):          # 3 images on a batch-2 plan (chunks of 2 + 1, of 4 for discriminate) against row-by-row calls
            one = run(which, x[i:i + 1], es[i:i + 1])
            assert all(same_bits(one[k], full[k][i:i + 1]) for k in full), f"{which}: row {i} depends on its batch"
    # eval-mode arithmetic whatever module.training says, and the flag is left alone
    net.train()
    tr = run("similarity", x, eps)
    assert all(same_bits(tr[k], eager["similarity"][k]) for k in tr) and net.training
    net.eval()
    # graph replay == eager, bit for bit, right after capture()
    inf.capture()
    assert {"gan.params", "gan.forward", "gan.discriminate", "gan.similarity"} <= set(inf._graphs)
    for which in eager:
        rep = run(which, x, zlat if which == "params" else eps)
        assert all(same_bits(rep[k], eager[which][k]) for k in rep), f"{which}: replayed differs from eager"
    # nothing above wrote to the module
    after, flags_after = R.state(net)
    assert flags_after == flags
    for k in before:
        assert torch.equal(before[k], after[k]), f"{k} was modified"

    # refresh(): the plan snapshots the model; after a change a stale plan is wrong, a refreshed one is a freshly built one
    with torch.no_grad():
        net.discriminator.conv[0][0].weight.mul_(1.25)
        net.discriminator.conv[1].conv.weight.mul_(0.8)
        net.discriminator.conv[1].bn.running_var.mul_(2.0)
        net.discriminator.fc[1].running_mean.add_(0.05)
        net.param_encoder.head[2].weight.mul_(1.5)
        net.param_encoder.r_fc[0].bias.add_(0.3)
    fresh_plan = V.FusedVAEGANInference(net, B)
    fresh = {w: run(w, x, zlat if w == "params" else eps, fresh_plan) for w in eager}
    stale = {w: run(w, x, zlat if w == "params" else eps) for w in eager}
    assert not same_bits(stale["params"]["params"], fresh["params"]["params"]), "a stale plan keeps the folded map it was built with"
    assert not same_bits(stale["similarity"]["mse"], fresh["similarity"]["mse"])
    inf.refresh()                                                  # (captured: the graphs are captured again)
    for w in eager:
        new = run(w, x, zlat if w == "params" else eps)
        assert all(same_bits(new[k], fresh[w][k]) for k in new), f"{w}: refresh() does not match a freshly built plan"


def test_error_paths():
    import vae_play_amd as V
    from vae_play_amd import _lib
    torch.manual_seed(0)
    net = V.VaeGan(16, 8).to(DEV).eval()
    inf = V.FusedVAEGANInference(net, 2)
    with pytest.raises(_lib.VaePlayHipError, match="shape"):
        inf.discriminate(torch.zeros((2, 1, 32, 32), device=DEV))
    with pytest.raises(_lib.VaePlayHipError, match="shape"):
        inf.params(torch.zeros((2, 9), device=DEV))
    with pytest.raises(_lib.VaePlayHipError, match="rows"):
        inf.similarity(torch.zeros((2, 1, 16, 16), device=DEV), eps=torch.zeros((3, 8), device=DEV))
    f32 = V.FusedVAEGANInference(net, 2, precision="f32")
    x = torch.rand((2, 1, 16, 16), device=DEV)
    xt, params = f32.forward(x, torch.zeros((2, 8), device=DEV))
    assert xt.shape == (2, 1, 16, 16) and params.shape == (2, 3) and same_bits(f32.params(f32.encode(x)[0]), params)
    with pytest.raises(NotImplementedError, match="bf16x3"):
        f32.similarity(x)
