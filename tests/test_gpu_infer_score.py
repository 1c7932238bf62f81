"""FusedVAEInference.score on the GPU: the per-image terms against the CPU oracle evaluated in fp64 (eval mode, the same eps), next
to the composed path -- the modules in ``.eval()``, then per-image BCE, KL, density ratio and log-sum-exp in ATen -- on the same
weights and inputs; and the properties that need no oracle (the decode of ``reconstruct``, chunking, graph replay, seeded draws, the
bound between its smallest and largest weight, purity, refresh()).

The models follow the recipe of tests/test_gpu_infer.py: gamma ~ U(0.5, 1.5) and beta ~ N(0, 0.2) from a seeded generator, then
three train-mode forwards on seeded batches, so that the eval state is not the trivial one.

Bound, as in that file: a term's error against fp64 is at most NORTH_STAR_RTOL and at most max(2 x the composed path's error, the
mode's FLOOR); here per image, |got - want| / |want| (every term has one sign and is far from zero: bce >= 1e2, kl > 0).
Precondition, asserted: the oracle's largest |logit| of x_tilde stays below 12, so neither fp32 saturation of the sigmoid nor the
-100 clamp plays a part in the comparison.

Measured on MI355X (worst over images, the two shapes and K = 1, 3; fused | composed; the oracle's largest |logit| was 1.64):
  f32     bce 1.3e-7 | 1.2e-7   kl 5.6e-7 | 7.4e-7   logw 1.6e-7 | 8.9e-8   elbo 1.5e-7 | 1.7e-7   iwae 1.3e-7 | 8.9e-8
  bf16x3  bce 1.2e-7 | 1.1e-7   kl 4.0e-6 | 4.1e-6   logw 1.6e-7 | 1.1e-7   elbo 1.7e-7 | 1.5e-7   iwae 1.6e-7 | 1.3e-7
(all at the rounding of a single fp32 value: the per-image sums average the per-pixel errors away; only the KL shows the mode)"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import score_ref as R
from tests.util import NORTH_STAR_RTOL, record

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = {"f32": 4e-6, "bf16x3": 1.4e-5}        # DESIGN.md section 3, as tests/test_gpu_infer.py
SHAPES = [(1, 32, 16, 4), (3, 64, 64, 4)]      # (C, S, z, B)
N, KMAX = 6, 3                                 # six images over batch size 4: a short last chunk
TERMS = ("bce", "kl", "logw", "elbo", "iwae")


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


def _batch(C, S, z, n=N, k=KMAX, seed=7):
    x = torch.rand((n, C, S, S), generator=torch.Generator().manual_seed(seed))
    eps = torch.randn((n, k, z), generator=torch.Generator().manual_seed(seed + 1))
    return x, eps


_MODEL, _ORACLE = {}, {}


def _model(C, S, z, B):
    """one trained model per shape, shared (and left unchanged) by the tests that only read it"""
    key = (C, S, z, B)
    if key not in _MODEL:
        _MODEL[key] = _trained_vae(C, S, z, B)
    return _MODEL[key]


def _terms64(bce, kl, lr):
    """the five terms in fp64 from bce (n, k), kl (n,), lr (n, k)"""
    logw, iwae = R.iw_bound(bce, lr)
    return {"bce": bce, "kl": kl, "logw": logw, "elbo": -(bce.mean(1) + kl), "iwae": iwae}


def _oracle(vae, C, S, z, B):
    """fp64 eval-mode forwards of the CPU oracle, one per draw, on the model's state: (bce (n, KMAX), kl, lr (n, KMAX), the largest
    |logit| of x_tilde); one evaluation per shape, both precisions and both K share it"""
    from oracle import ref_cpu as O
    key = (C, S, z, B)
    if key not in _ORACLE:
        p64 = {k: (v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu().clone()) for k, v in vae.state_dict().items()}
        x, eps = _batch(C, S, z)
        bce, lr, logit = [], [], 0.0
        with torch.no_grad():
            for j in range(KMAX):
                out = O.vae_forward(p64, x.double(), eps[:, j].double(), vae.iter_level, training=False)
                bce.append(R.bce_rows(out["x_tilde"], x))
                lr.append(R.latent_iw(out["mu"], out["logvar"], eps[:, j])[2])
                logit = max(logit, float(torch.logit(out["x_tilde"]).abs().max()))
            kl = O.kl_per_sample(out["mu"], out["logvar"])
        _ORACLE[key] = (torch.stack(bce, 1), kl, torch.stack(lr, 1), logit)
    return _ORACLE[key]


def _composed(vae, x, eps, prec):
    """the path a user has without ``score``: the modules in eval mode, one forward per draw (the encoder runs again each time),
    then the terms in ATen, fp32"""
    import vae_play_amd as V
    n, k, _ = eps.shape
    V.set_conv_precision(prec)
    try:
        with torch.no_grad():
            bce, lr = [], []
            for j in range(k):
                xt, mu, logvar = vae(x, eps[:, j].contiguous())
                bce.append(F.binary_cross_entropy(xt, x, reduction="none").flatten(1).sum(1))
                zz = eps[:, j] * torch.exp(0.5 * logvar) + mu
                lr.append(-0.5 * (zz * zz).sum(1) + 0.5 * (eps[:, j] ** 2 + logvar).sum(1))
            bce, lr = torch.stack(bce, 1), torch.stack(lr, 1)
            kl = -0.5 * (1.0 + logvar - mu * mu - torch.exp(logvar)).sum(1)
            logw = lr - bce
            return {"bce": bce, "kl": kl, "logw": logw, "elbo": -(bce.mean(1) + kl), "iwae": torch.logsumexp(logw, 1) - math.log(k)}
    finally:
        V.set_conv_precision("f32")


def _per_image_err(got, want):
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return ((got - want).abs() / want.abs()).max().item()


@pytest.mark.parametrize("k", (1, KMAX))
@pytest.mark.parametrize("C,S,z,B", SHAPES)
@pytest.mark.parametrize("prec", ("bf16x3", "f32"))
def test_score_vs_fp64_oracle(prec, C, S, z, B, k):
    import vae_play_amd as V
    vae = _model(C, S, z, B)
    bce64, kl64, lr64, logit = _oracle(vae, C, S, z, B)
    print(f"{S}x{S}x{C}: largest |logit| of the oracle's x_tilde {logit:.2f}")
    assert logit < 12.0, f"largest |logit| {logit:.2f}: the sigmoid saturates in fp32, pick another seed"
    want = _terms64(bce64[:, :k], kl64, lr64[:, :k])
    assert float(want["bce"].min()) > 1e2 and float(want["kl"].min()) > 0.0
    x, eps = _batch(C, S, z)
    x, eps = x.to(DEV), eps[:, :k].contiguous().to(DEV)
    inf = V.FusedVAEInference(vae, B, S, C, precision=prec)
    got = inf.score(x, k, eps)
    mod = _composed(vae, x, eps, prec)
    torch.cuda.synchronize()
    assert set(got) == set(TERMS)
    assert got["bce"].shape == (N, k) and got["logw"].shape == (N, k) and all(got[t].shape == (N,) for t in ("kl", "elbo", "iwae"))
    tag = f"{prec} {S}x{S}x{C} b{B} n{N} k{k}"
    fails = []
    for name in TERMS:
        ef, em = _per_image_err(got[name], want[name]), _per_image_err(mod[name], want[name])
        record(f"score fused {tag} {name}", ef)
        record(f"score composed {tag} {name}", em)
        print(f"{tag} {name}: fused {ef:.3e}  composed {em:.3e}")
        if not ef <= NORTH_STAR_RTOL:
            fails.append(f"{name}: fused {ef:.3e} > {NORTH_STAR_RTOL:.0e}")
        if not ef <= max(2 * em, FLOOR[prec]):
            fails.append(f"{name}: fused {ef:.3e} > max(2 x composed {em:.3e}, floor {FLOOR[prec]:.1e})")
    assert not fails, "; ".join(fails)
    assert vae.training is False


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[t], b[t]) for t in a)


def _state(vae):
    return {k: v.detach().clone() for k, v in vae.state_dict().items()}, {n: m.training for n, m in vae.named_modules()}


@pytest.mark.parametrize("C,S,z,B", SHAPES)
@pytest.mark.parametrize("prec", ("bf16x3", "f32"))
def test_properties_without_oracle(prec, C, S, z, B):
    import vae_play_amd as V
    from vae_play_amd import ops
    vae = _trained_vae(C, S, z, B, seed=1)         # (its own model: the end of this test changes weights)
    before, flags = _state(vae)
    inf = V.FusedVAEInference(vae, B, S, C, precision=prec)
    bufs_before = dict(inf._bufs)
    x, eps = _batch(C, S, z)
    x, eps = x.to(DEV), eps.to(DEV)
    eps1 = eps[:, :1].contiguous()

    # one draw: the decode IS reconstruct's, the terms are the kernels' on it
    s1 = inf.score(x, 1, eps1)
    xt, mu, logvar = inf.reconstruct(x, eps1[:, 0])
    assert torch.equal(s1["bce"][:, 0], ops.bce_rows(xt, x))
    assert torch.equal(s1["kl"], ops.latent_fwd(mu, logvar, eps1[:, 0].contiguous())[1])
    assert torch.equal(s1["iwae"], s1["logw"][:, 0]) and torch.equal(s1["elbo"], -(s1["bce"][:, 0] + s1["kl"]))
    # scoring allocated its own buffers and left every other one alone
    assert {n: t.data_ptr() for n, t in inf._bufs.items() if not n.startswith("score.")} == {n: t.data_ptr() for n, t in bufs_before.items()}
    # three draws: draw 0 is the one-draw score; the bound lies between the smallest and the largest weight
    s3 = inf.score(x, KMAX, eps)
    assert torch.equal(s3["bce"][:, 0], s1["bce"][:, 0]) and torch.equal(s3["logw"][:, 0], s1["logw"][:, 0]) and torch.equal(s3["kl"], s1["kl"])
    assert (s3["iwae"] >= s3["logw"].min(1).values).all() and (s3["iwae"] <= s3["logw"].max(1).values).all()
    assert not torch.equal(s3["bce"][:, 1], s3["bce"][:, 0])
    # two runs give the same bits (after a larger k_max replaced the buffers, too)
    assert _same(inf.score(x, KMAX, eps), s3) and _same(inf.score(x, 1, eps1), s1)
    # chunking: 6 images over batch size 4 == rows 0:4 and 4:6 on their own
    for k, e, full in ((1, eps1, s1), (KMAX, eps, s3)):
        a, b = inf.score(x[0:4], k, e[0:4]), inf.score(x[4:6], k, e[4:6])
        assert _same({t: torch.cat([a[t], b[t]]) for t in a}, full), f"k = {k}: chunks differ from the whole"
    # no eps: drawn from the generator, reproducibly, as (n, k, Z)
    g = torch.Generator(device=DEV)
    ra, rb = inf.score(x, 2, generator=g.manual_seed(3)), inf.score(x, 2, generator=g.manual_seed(3))
    rc = inf.score(x, 2, eps=torch.randn((N, 2, z), device=DEV, generator=g.manual_seed(3)))
    assert _same(ra, rb) and _same(ra, rc) and torch.equal(ra["kl"], s1["kl"]) and not torch.equal(ra["bce"], s3["bce"][:, :2])
    # eval-mode arithmetic whatever module.training says
    vae.train()
    assert _same(inf.score(x, KMAX, eps), s3) and vae.training
    vae.eval()

    # graph replay == eager, bit for bit: the lists built before capture(), and one built after it
    eager4 = V.FusedVAEInference(vae, B, S, C, precision=prec).score(x, 4, torch.cat([eps, eps1], 1))
    inf.capture()
    assert {"score1", "score2", f"score{KMAX}"} <= set(inf._graphs)
    assert _same(inf.score(x, 1, eps1), s1) and _same(inf.score(x, KMAX, eps), s3) and _same(inf.score(x, 2, generator=g.manual_seed(3)), ra)
    assert torch.equal(inf.reconstruct(x, eps1[:, 0])[0], xt)
    assert _same(inf.score(x, 4, torch.cat([eps, eps1], 1)), eager4) and "score4" in inf._graphs
    assert _same(inf.score(x, KMAX, eps), s3)                  # (k_max grew to 4: new buffers, lists and graphs)

    # nothing above wrote to the module
    after, flags_after = _state(vae)
    assert flags_after == flags
    for key in before:
        assert torch.equal(before[key], after[key]), f"{key} was modified"

    # refresh(): a stale plan keeps its weights, refresh() picks the change up, restoring them restores the bits
    w = vae.decoder.conv[1].conv.weight
    saved = w.detach().clone()
    with torch.no_grad():
        w.mul_(1.5)
    assert _same(inf.score(x, KMAX, eps), s3), "a stale plan must not see the change"
    inf.refresh()
    s_new = inf.score(x, KMAX, eps)
    assert not torch.equal(s_new["bce"], s3["bce"]) and torch.equal(s_new["kl"], s3["kl"])      # (a decoder weight: the KL stays)
    with torch.no_grad():
        w.copy_(saved)
    inf.refresh()
    assert _same(inf.score(x, KMAX, eps), s3)


def test_error_paths():
    """host-side validation only"""
    import vae_play_amd as V
    from vae_play_amd import _lib
    torch.manual_seed(0)
    vae = V.VAE(32, 16, 1).to(DEV).eval()
    inf = V.FusedVAEInference(vae, 4, 32, 1)
    x = torch.zeros((2, 1, 32, 32), device=DEV)
    with pytest.raises(_lib.VaePlayHipError, match="shape"):
        inf.score(torch.zeros((2, 3, 32, 32), device=DEV))
    with pytest.raises(_lib.VaePlayHipError, match="shape"):
        inf.score(x, 2, eps=torch.zeros((2, 16), device=DEV))              # (n, Z): reconstruct's, not score's
    with pytest.raises(_lib.VaePlayHipError, match="shape"):
        inf.score(x, 2, eps=torch.zeros((2, 3, 16), device=DEV))           # k
    with pytest.raises(_lib.VaePlayHipError, match="fp32"):
        inf.score(x, 1, eps=torch.zeros((2, 1, 16), device=DEV, dtype=torch.float64))
    with pytest.raises(_lib.VaePlayHipError, match="HIP device"):
        inf.score(x, 1, eps=torch.zeros((2, 1, 16)))
    with pytest.raises(_lib.VaePlayHipError, match="rows"):
        inf.score(x, 1, eps=torch.zeros((3, 1, 16), device=DEV))
    with pytest.raises(ValueError):
        inf.score(x, 0)
    assert inf._score is None and set(inf._plans) == {"encode", "decode", "reconstruct"}      # a refused call builds nothing
