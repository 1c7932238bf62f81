"""FusedVAEInference.decode_grad / project on the GPU: the decoder's input gradient against the fp64 restatement of
tests/project_ref.py by the method and with the constants of tests/test_gpu_grad_accuracy.py (ReLU-mask flips counted and bounded;
given the same masks the gradient is as good as fp32 arithmetic allows), and the properties that need no oracle: masked pixels carry
nothing, project() is decode_grad + the latent update composed, graph replay, chunking, row independence, that it optimises,
purity and refresh().

Models have non-trivial eval state, made as tests/test_gpu_infer.py::_trained_vae makes its own (gamma ~ U(0.5, 1.5), beta ~ N(0, 0.2),
three train-mode forwards at momentum 0.9) -- by the CPU oracle on the host (tests/project_ref.py::trained_params) and loaded into
the module, so that the condition test_it_optimises stands on is checked without a GPU on the very same model
(tests/test_infer_project_plan_cpu.py::test_ref_project_loop_lowers_the_loss)."""
import pytest
import torch

from tests import project_ref as R
from tests.test_gpu_grad_accuracy import GRAD_FLOOR, U_MODE
from tests.test_gpu_infer import FLOOR
from tests.util import NORTH_STAR_RTOL, RAW_GRAD_L2, record, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 16, 8, 2), (3, 32, 16, 2), (3, 64, 64, 4)]      # (C, S, z, B)
SMALL = SHAPES[:2]
_MODELS, _REFS = {}, {}


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _trained_vae(C, S, z, B):
    """(module in eval mode on the device, its state in fp64 and fp32 on the host, L); one model per shape"""
    import vae_play_amd as V
    key = (C, S, z, B)
    if key not in _MODELS:
        p32, L = R.trained_params(C, S, z, B)
        _MODELS[key] = (p32, R.cast_params(p32, torch.float64), L)
    p32, p64, L = _MODELS[key]
    vae = V.VAE(S, z, C, init_rule=False)
    vae.load_state_dict(p32)
    return vae.to(DEV).eval(), p64, p32, L


def _inputs(C, S, z, n, seed=11):
    g = torch.Generator().manual_seed(seed)
    zz, x = torch.randn(n, z, generator=g), torch.rand(n, C, S, S, generator=g)
    mask = torch.rand(n, C, S, S, generator=g) * (torch.rand(n, C, S, S, generator=g) > 0.3)      # weights in [0, 1], 30 % exact zeros
    return zz, x, mask


def _refs(key, p64, p32, L, zz, x, mask, pw):
    """fp64 and fp32 evaluations with their own masks, once per (shape, mask?, prior weight): both precisions share them"""
    k = key + (mask is not None, pw)
    if k not in _REFS:
        _REFS[k] = (R.decode_grad(p64, zz, x, L, mask, pw), R.decode_grad(p32, zz, x, L, mask, pw))
    return _REFS[k]


def _hip_masks(inf):
    """ReLU masks of the plan's decode pass, in project_ref's layer order and shapes"""
    from vae_play_amd import ops
    bufs, B = inf._bufs, inf.B
    out = [(bufs["dec.db"].view(B, -1) > 0).cpu()]
    for i in range(inf.L):
        Cout, Hs = inf.decoder.conv[i].conv.weight.shape[1], 16 << i
        n = B * Hs * Hs * Cout
        a = bufs[f"dec{i}.u"].flatten()[:n] if f"dec{i}.u" in bufs else ops.unsplit(bufs[f"dec{i}.us"])[:n]
        out.append((a.view(B, Hs, Hs, Cout).permute(0, 3, 1, 2) > 0).cpu())
    return out


# ---- (a) decode_grad against fp64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,S,z,B", SHAPES)
@pytest.mark.parametrize("prec", ("bf16x3", "f32"))
def test_decode_grad_against_fp64(prec, C, S, z, B):
    import vae_play_amd as V
    vae, p64, p32, L = _trained_vae(C, S, z, B)
    inf = V.FusedVAEInference(vae, B, S, C, precision=prec)
    zz, x, mask = _inputs(C, S, z, B)
    tag = f"project {prec} {S}x{S}x{C} b{B}"
    fails = []
    for mk in (None, mask):
        for pw in (0.0, 1.0):
            g64, g32 = _refs((C, S, z, B), p64, p32, L, zz, x, mk, pw)
            out = inf.decode_grad(zz.to(DEV), x.to(DEV), None if mk is None else mk.to(DEV), pw)
            torch.cuda.synchronize()
            what = f"{tag} mask={mk is not None} pw={pw:g}"
            # ReLU masks: how many units did rounding put on the other side of zero?
            mh = _hip_masks(inf)
            assert [tuple(m.shape) for m in mh] == [tuple(m.shape) for m in g64["masks"]]
            units = sum(m.numel() for m in mh)
            flips = sum(int((a != (b > 0)).sum()) for a, b in zip(mh, g64["masks"]))
            record(f"{what} relu_mask_flips", flips)
            assert flips <= max(4, 8 * U_MODE[prec] * units), f"{what}: {flips} of {units} ReLU masks differ from the fp64 forward pass"
            g64m = R.decode_grad(p64, zz, x, L, mk, pw, masks=[m.double() for m in mh]) if flips else g64
            # the gradient, given the same masks
            e_hip, e_raw, e_o32 = _rel(out["dz"], g64m["dz"]), _rel(out["dz"], g64["dz"]), _rel(g32["dz"], g64["dz"])
            record(f"{what} dz_vs_fp64_same_masks", e_hip)
            record(f"{what} dz_vs_fp64", e_raw)
            record(f"{what} oracle32_dz_vs_fp64", e_o32)
            print(f"{what}: dz {e_hip:.3e} (own masks {e_raw:.3e}, fp32 oracle {e_o32:.3e}), {flips} flips of {units}")
            if not e_hip <= max(2 * e_o32, GRAD_FLOOR[prec]):
                fails.append(f"{what}: dz {e_hip:.2e} vs fp64 with the same masks > max(2 x {e_o32:.2e}, {GRAD_FLOOR[prec]:.0e})")
            # the forward side: the image, and the per-image sums relative to themselves
            for name, got, want, want32 in (("x_tilde", out["x_tilde"], g64["x_tilde"], g32["x_tilde"]),):
                ef, e32 = rel_err(got, want), rel_err(want32, want)
                record(f"{what} {name}", ef)
                print(f"{what}: {name} {ef:.3e} (fp32 oracle {e32:.3e})")
                if not (ef <= NORTH_STAR_RTOL and ef <= max(2 * e32, FLOOR[prec])):
                    fails.append(f"{what}: {name} {ef:.3e} > max(2 x fp32 oracle {e32:.3e}, floor {FLOOR[prec]:.1e})")
            for name in ("bce", "loss"):
                got, want, want32 = out[name].cpu().double(), g64[name], g32[name].double()
                ef, e32 = ((got - want).abs() / want.abs()).max().item(), ((want32 - want).abs() / want.abs()).max().item()
                record(f"{what} {name}", ef)
                print(f"{what}: {name} {ef:.3e} (fp32 oracle {e32:.3e})")
                if not (ef <= NORTH_STAR_RTOL and ef <= max(2 * e32, FLOOR[prec])):
                    fails.append(f"{what}: {name} {ef:.3e} > max(2 x fp32 oracle {e32:.3e}, floor {FLOOR[prec]:.1e})")
    assert not fails, "\n".join(fails)


# ---- (b) .. (f): properties -------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)


def _state(vae):
    return {k: v.detach().clone() for k, v in vae.state_dict().items()}, {n: m.training for n, m in vae.named_modules()}


@pytest.mark.parametrize("C,S,z,B", SMALL)
@pytest.mark.parametrize("prec", ("bf16x3", "f32"))
def test_masked_pixels_composition_replay_and_chunking(prec, C, S, z, B):
    import vae_play_amd as V
    from vae_play_amd import ops
    vae, p64, p32, L = _trained_vae(C, S, z, B)
    before, flags = _state(vae)
    inf = V.FusedVAEInference(vae, B, S, C, precision=prec)
    zz, x, mask = (t.to(DEV) for t in _inputs(C, S, z, B))
    lr, pw, betas, eps, steps = 0.05, 0.5, (0.9, 0.999), 1e-8, 4

    # (b) masked pixels carry nothing: another x where mask == 0 gives the same bits
    g0 = inf.decode_grad(zz, x, mask, pw)
    x2 = torch.where(mask == 0, 1.0 - x, x)
    assert not torch.equal(x2, x)
    g1 = inf.decode_grad(zz, x2, mask, pw)
    assert torch.equal(g1["dz"], g0["dz"]) and torch.equal(g1["bce"], g0["bce"]) and torch.equal(g1["loss"], g0["loss"])
    assert not torch.equal(inf.decode_grad(zz, x2, None, pw)["dz"], inf.decode_grad(zz, x, None, pw)["dz"])
    # no mask is a mask of ones
    assert _same(inf.decode_grad(zz, x, None, pw), inf.decode_grad(zz, x, torch.ones_like(x), pw))

    # (c) composition: project() is `steps` rounds of decode_grad followed by the ops-level latent update on the plan's own buffers
    r = inf.project(x, steps=steps, lr=lr, mask=mask, z0=zz, prior_weight=pw, betas=betas, eps=eps, history=True)
    q = inf._proj
    zc = zz.clone()
    q.m.zero_()
    q.v.zero_()
    q.step.zero_()
    for i in range(steps):
        gi = inf.decode_grad(zc, x, mask, pw)
        assert torch.equal(r["history"][i], gi["loss"]), f"history[{i}] is not the loss of round {i}"
        ops.latent_adam_step(inf.z, q.dz, q.m, q.v, q.step, lr, betas[0], betas[1], eps, pw)
        zc = inf.z.clone()
    assert int(q.step.item()) == steps
    assert torch.equal(r["z"], zc), "project() differs from decode_grad + latent update composed"
    gf = inf.decode_grad(zc, x, mask, pw)
    assert torch.equal(r["loss"], gf["loss"]) and torch.equal(r["x_tilde"], gf["x_tilde"])
    # a second call starts from step 1 again: the same bits, whatever the state left behind
    assert _same(inf.project(x, steps=steps, lr=lr, mask=mask, z0=zz, prior_weight=pw, betas=betas, eps=eps, history=True), r)
    # zero steps: the loss at z0
    r0 = inf.project(x, steps=0, lr=lr, mask=mask, z0=zz, prior_weight=pw)
    assert torch.equal(r0["z"], zz) and torch.equal(r0["loss"], g0["loss"])

    # (d) chunking and independence: 3 images on a batch_size = 2 plan == row by row; z0 as a tensor == z0 = "encode"
    n = B + 1
    z3, x3, m3 = (t.to(DEV) for t in _inputs(C, S, z, n, seed=12))
    kw = dict(steps=3, lr=lr, prior_weight=pw, history=True)
    full = inf.project(x3, mask=m3, z0=z3, **kw)
    assert full["history"].shape == (3, n) and full["z"].shape == (n, z)
    rows = [inf.project(x3[i:i + 1], mask=m3[i:i + 1], z0=z3[i:i + 1], **kw) for i in range(n)]
    for k in ("z", "x_tilde", "loss"):
        assert torch.equal(full[k], torch.cat([ri[k] for ri in rows])), f"{k}: a row depends on its chunk"
    assert torch.equal(full["history"], torch.cat([ri["history"] for ri in rows], 1))
    gd = inf.decode_grad(z3, x3, m3, pw)
    assert _same(gd, {k: torch.cat([inf.decode_grad(z3[i:i + 1], x3[i:i + 1], m3[i:i + 1], pw)[k] for i in range(n)]) for k in gd})
    enc = inf.project(x3, mask=m3, z0="encode", **kw)
    assert _same(enc, inf.project(x3, mask=m3, z0=inf.encode(x3)[0], **kw))
    assert not torch.equal(enc["z"], full["z"])

    # graph replay == eager, bit for bit, also with other hyper-parameters (the lists that carry them are captured again)
    inf.capture()
    assert _same(inf.project(x, steps=steps, lr=lr, mask=mask, z0=zz, prior_weight=pw, betas=betas, eps=eps, history=True), r)
    assert _same(inf.project(x3, mask=m3, z0=z3, **kw), full) and _same(inf.decode_grad(z3, x3, m3, pw), gd)
    eager = V.FusedVAEInference(vae, B, S, C, precision=prec).project(x, steps=2, lr=0.1, mask=mask, z0="zeros", prior_weight=1.0)
    assert _same(inf.project(x, steps=2, lr=0.1, mask=mask, z0="zeros", prior_weight=1.0), eager)

    # (f) nothing above wrote to the module
    after, flags_after = _state(vae)
    assert flags_after == flags
    for k in before:
        assert torch.equal(before[k], after[k]), f"{k} was modified"


@pytest.mark.parametrize("C,S,z,B", SMALL)
@pytest.mark.parametrize("prec", ("bf16x3", "f32"))
def test_it_optimises(prec, C, S, z, B):
    """(e) from zeros, 20 steps at lr 0.05 towards the model's own decode of a seeded z*: every image's loss ends below where it
    started -- on the plan, and (the condition this stands on) in the fp64 loop of tests/project_ref.py on the same target"""
    import vae_play_amd as V
    vae, p64, p32, L = _trained_vae(C, S, z, B)
    inf = V.FusedVAEInference(vae, B, S, C, precision=prec)
    x = inf.decode(R.z_star(B, z).to(DEV))
    zf, hist = R.project(p64, x.cpu().double(), L, torch.zeros(B, z, dtype=torch.float64), 20, 0.05)
    final = R.decode_grad(p64, zf, x.cpu().double(), L, None, 1.0)["loss"]
    assert (final < hist[0]).all(), f"the fp64 loop does not lower the loss: {hist[0].tolist()} -> {final.tolist()}"
    r = inf.project(x, steps=20, lr=0.05, z0="zeros", history=True)
    print(f"{prec} {S}x{S}x{C}: loss {r['history'][0].tolist()} -> {r['loss'].tolist()} (fp64: {hist[0].tolist()} -> {final.tolist()})")
    assert (r["loss"] < r["history"][0]).all(), (r["history"][0], r["loss"])
    assert (r["history"][-1] < r["history"][0]).all()
    assert rel_err(r["history"][0], hist[0]) <= NORTH_STAR_RTOL            # both start from the loss at zero


@pytest.mark.parametrize("prec", ("bf16x3", "f32"))
def test_refresh(prec):
    """(f) a stale plan keeps the weights it was built with; refresh() makes decode_grad follow the new model (eager and replayed)"""
    import vae_play_amd as V
    C, S, z, B = SMALL[1]
    vae, p64, p32, L = _trained_vae(C, S, z, B)
    inf = V.FusedVAEInference(vae, B, S, C, precision=prec)
    zz, x, mask = _inputs(C, S, z, B)
    zd, xd, md = zz.to(DEV), x.to(DEV), mask.to(DEV)
    g_old = inf.decode_grad(zd, xd, md, 1.0)
    inf.capture()
    w, bn = vae.decoder.conv[0].conv.weight, vae.decoder.conv[1].bn
    saved_w, saved_rv = w.detach().clone(), bn.running_var.clone()
    with torch.no_grad():
        w.mul_(1.5)
        bn.running_var.mul_(2.0)
    assert _same(inf.decode_grad(zd, xd, md, 1.0), g_old), "a stale plan must not see the change"
    inf.refresh()
    g_new = inf.decode_grad(zd, xd, md, 1.0)
    want = R.decode_grad(R.cast_params(vae.state_dict(), torch.float64), zz, x, L, mask, 1.0)
    e_new, e_old = _rel(g_new["dz"], want["dz"]), _rel(g_old["dz"], want["dz"])
    print(f"refresh {prec}: dz of the refreshed plan {e_new:.3e} from the new model, of the stale plan {e_old:.3e}")
    assert e_new <= RAW_GRAD_L2[prec] and e_old > 10 * RAW_GRAD_L2[prec], (e_new, e_old)
    with torch.no_grad():
        w.copy_(saved_w)
        bn.running_var.copy_(saved_rv)
    inf.refresh()
    assert _same(inf.decode_grad(zd, xd, md, 1.0), g_old)


def test_error_paths():
    """host-side validation only"""
    import vae_play_amd as V
    from vae_play_amd import _lib
    C, S, z, B = SMALL[0]
    vae, _, _, _ = _trained_vae(C, S, z, B)
    inf = V.FusedVAEInference(vae, B, S, C)
    x, zz = torch.rand(2, C, S, S, device=DEV), torch.zeros(2, z, device=DEV)
    with pytest.raises(_lib.VaePlayHipError, match="shape"):
        inf.project(x, mask=torch.ones(2, C, S, S // 2, device=DEV))
    with pytest.raises(_lib.VaePlayHipError, match="rows"):
        inf.project(x, mask=torch.ones(3, C, S, S, device=DEV))
    with pytest.raises(_lib.VaePlayHipError, match="rows"):
        inf.project(x, z0=torch.zeros(3, z, device=DEV))
    with pytest.raises(_lib.VaePlayHipError, match="rows"):
        inf.decode_grad(torch.zeros(3, z, device=DEV), x)
    with pytest.raises(_lib.VaePlayHipError, match="fp32"):
        inf.decode_grad(zz, x, mask=torch.ones(2, C, S, S, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError):
        inf.project(x, z0="mean")
    with pytest.raises(ValueError):
        inf.project(x, steps=-1)
    with pytest.raises(ValueError):
        inf.decode_grad(zz, x, prior_weight=-1.0)
    with pytest.raises(NotImplementedError):
        V.FusedVAEInference(vae, B, S, C, precision="f16").project(x)
