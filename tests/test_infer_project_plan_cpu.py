"""Latent projection on the fused inference plan (FusedVAEInference.project / decode_grad), checked without a GPU: the restatements
of tests/project_ref.py against the CPU oracle's eval-mode decoder under torch autograd and against torch.optim.Adam, the ABI table,
and the structure of the lazily built projection lists over host buffers (``_plan_only=True``; nothing is run)."""
import gc
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import project_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import gen_golden_fused_plans as G  # noqa: E402  (the canonical form of a launch list)

PROJECT_SYMBOLS = ("vp_affine_relu_bwd_f32", "vp_bce_masked_rows_bwd_workspace_bytes", "vp_bce_masked_rows_bwd_f32", "vp_latent_adam_f32")
CASES = [(prec, C, S, z, B) for prec in ("bf16x3", "f32") for (C, S, z, B) in ((1, 16, 8, 2), (3, 32, 16, 2))]
OLD = ("encode", "decode", "reconstruct")
NEW = ("project", "project.grad", "project.loss")           # and "project.load" (target and mask to NHWC) for more than one channel


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


# ---- the references -----------------------------------------------------------------------------------------------------------
def _oracle_model(C, S, z, B=2, seed=0):
    """the oracle-trained model of tests/project_ref.py (non-trivial eval-mode BatchNorm constants), in fp64"""
    p, L = R.trained_params(C, S, z, B, seed)
    return R.cast_params(p, torch.float64), L


@pytest.mark.parametrize("C,S,z", [(1, 16, 8), (3, 32, 16)])
def test_ref_decode_grad_is_the_oracle_decoder_under_autograd(C, S, z):
    from oracle import ref_cpu as O
    p, L = _oracle_model(C, S, z)
    g = _gen(3)
    n = 3
    zz = torch.randn(n, z, generator=g, dtype=torch.float64)
    x = torch.rand(n, C, S, S, generator=g, dtype=torch.float64)
    mask = (torch.rand(n, C, S, S, generator=g) > 0.3).double() * torch.rand(n, C, S, S, generator=g, dtype=torch.float64)
    for m, pw in ((None, 0.0), (mask, 0.0), (mask, 1.0), (None, 0.7)):
        got = R.decode_grad(p, zz, x, L, m, pw)
        zr = zz.clone().requires_grad_(True)
        xt = O.decoder_forward(p, zr, L, training=False)
        w = torch.ones_like(x) if m is None else m
        bce = (w * F.binary_cross_entropy(xt, x, reduction="none")).reshape(n, -1).sum(1)
        loss = bce + 0.5 * pw * (zr * zr).sum(1)
        (dz,) = torch.autograd.grad(loss.sum(), zr)
        assert _rel(got["x_tilde"], xt.detach()) < 1e-12 and _rel(got["bce"], bce.detach()) < 1e-12
        assert _rel(got["loss"], loss.detach()) < 1e-12 and _rel(got["dz"], dz) < 1e-12
        # the masks are the ReLU's, in layer order; given back they reproduce the same numbers
        assert [tuple(k.shape) for k in got["masks"]][0] == (n, p["decoder.fc.0.weight"].shape[0]) and len(got["masks"]) == L + 1
        again = R.decode_grad(p, zz, x, L, m, pw, masks=got["masks"])
        assert torch.equal(again["dz"], got["dz"]) and torch.equal(again["bce"], got["bce"])
        # ... and the kernel formulas agree with it: the BCE rows, and dlogit as the gradient at the logits
        out, dl = R.bce_masked_rows(xt.detach(), x, m)
        assert _rel(out, bce.detach()) < 1e-12
        logit = torch.logit(xt.detach()).requires_grad_(True)
        (want,) = torch.autograd.grad((w * F.binary_cross_entropy(torch.sigmoid(logit), x, reduction="none")).sum(), logit)
        assert _rel(dl, want) < 1e-9            # (through logit / sigmoid, which round)


def test_ref_affine_relu_bwd_is_autograd_through_the_folded_block():
    g = _gen(4)
    c, dy = torch.randn(37, 24, generator=g, dtype=torch.float64), torch.randn(37, 24, generator=g, dtype=torch.float64)
    s, t = torch.rand(24, generator=g, dtype=torch.float64) + 0.5, torch.randn(24, generator=g, dtype=torch.float64)
    s[3] = -s[3]                # a negative BatchNorm weight: the mask is still the output's
    cr = c.clone().requires_grad_(True)
    u = F.relu(s * cr + t)
    (want,) = torch.autograd.grad(u, cr, dy)
    assert _rel(R.affine_relu_bwd(dy, u.detach(), s), want) < 1e-14


@pytest.mark.parametrize("pw", (0.0, 1.0))
def test_ref_latent_adam_is_torch_adam(pw):
    g = _gen(5)
    lr, betas, eps = 0.05, (0.9, 0.999), 1e-8
    z = torch.randn(4, 9, generator=g, dtype=torch.float64)
    zt = z.clone().requires_grad_(True)
    opt = torch.optim.Adam([zt], lr=lr, betas=betas, eps=eps)
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    for step in range(1, 5):
        gr = torch.randn(4, 9, generator=g, dtype=torch.float64)
        zt.grad = gr + pw * zt.detach()
        opt.step()
        z_in = z
        z, m, v, prior = R.latent_adam(z, gr, m, v, step, lr, betas[0], betas[1], eps, pw)
        torch.testing.assert_close(z, zt.detach(), rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(prior, 0.5 * pw * (z_in * z_in).sum(1), rtol=1e-14, atol=0)


@pytest.mark.parametrize("C,S,z,B", [(1, 16, 8, 2), (3, 32, 16, 2)])
def test_ref_project_loop_lowers_the_loss(C, S, z, B):
    """the condition tests/test_gpu_infer_project.py::test_it_optimises stands on, on the same model, targets and settings: from zeros,
    20 steps at lr 0.05 towards the model's own decode of a seeded z*, every image's loss ends below where it started"""
    p, L = _oracle_model(C, S, z, B)
    x = R.decoder_masked(p, R.z_star(B, z).double(), L)[0].float().double()
    zf, hist = R.project(p, x, L, torch.zeros(B, z, dtype=torch.float64), 20, 0.05)
    final = R.decode_grad(p, zf, x, L, None, 1.0)["loss"]
    assert hist.shape == (20, B) and (final < hist[0]).all(), (hist[0], final)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_table_carries_the_projection_entry_points():
    from vae_play_amd import _lib
    lib = _lib.load()
    for name in PROJECT_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for rows, n in ((3, 1), (3, 4096), (3, 4097), (32, 49152), (0, 5), (5, 0)):
        assert lib.vp_bce_masked_rows_bwd_workspace_bytes(rows, n) == lib.vp_bce_rows_workspace_bytes(rows, n)


# ---- the plan -----------------------------------------------------------------------------------------------------------------
def _build(prec, C, S, z, B):
    import vae_play_amd as V
    torch.manual_seed(0)
    vae = V.VAE(S, z, C)
    return vae, V.FusedVAEInference(vae, B, S, C, precision=prec, _plan_only=True)


def _record(vae, inf, which):
    """canonical form of the lists ``which`` of a plan (pointers as [owner, ordinal, offset]) and the number of pointers nobody owns"""
    plans, seen = [("prep", inf._prep)], {}
    for w in which:
        for p in inf._plans[w]:
            seen.setdefault(id(p), (p, []))[1].append(w)
    plans += [("+".join(names), p) for p, names in seen.values()]
    if inf._proj is not None:       # (last: buffers are numbered by first appearance)
        plans.append(("project.prep", inf._proj.prep))
    calls, unknown, _ = G.canonical(inf, plans, [("", vae)], {})
    return calls, unknown


def _shapes(inf):
    return {n: (tuple(t.shape), t.dtype) for n, t in inf._bufs.items()}


@pytest.mark.parametrize("prec,C,S,z,B", CASES)
def test_a_plan_that_never_projects_is_untouched(prec, C, S, z, B):
    import vae_play_amd as V
    torch.manual_seed(0)
    vae = V.VAE(S, z, C)
    plain = V.FusedVAEInference(vae, B, S, C, precision=prec, _plan_only=True)
    proj = V.FusedVAEInference(vae, B, S, C, precision=prec, _plan_only=True)
    assert plain._proj is None and set(plain._plans) == set(OLD) and not any(n.startswith("project") for n in plain._bufs)
    before = _shapes(proj)
    assert before == _shapes(plain) and list(before) == list(plain._bufs)
    lists_before = {w: [id(p) for p in proj._plans[w]] for w in OLD}
    ptrs_before = {n: t.data_ptr() for n, t in proj._bufs.items()}
    proj.enable_projection()
    proj.enable_projection()                    # (a second call changes nothing)
    # the old buffers are the same tensors, the old lists the same objects; what is new is named project.*
    assert {n: v for n, v in _shapes(proj).items() if not n.startswith("project.")} == before
    assert [n for n in proj._bufs if not n.startswith("project.")] == list(before)
    assert {n: t.data_ptr() for n, t in proj._bufs.items() if not n.startswith("project.")} == ptrs_before
    assert {w: [id(p) for p in proj._plans[w]] for w in OLD} == lists_before
    assert set(proj._plans) == set(OLD) | set(NEW) | ({"project.load"} if C > 1 else set())
    # ... with the same launches, argument for argument, as the plan that never heard of projection
    gc.collect()
    want, got = _record(vae, plain, OLD), _record(vae, proj, OLD)
    strip = lambda calls: [c for c in calls if c[0] != "project.prep"]      # noqa: E731
    assert want[1] == 0 and got[1] == 0 and strip(got[0]) == want[0]


@pytest.mark.parametrize("prec,C,S,z,B", CASES)
def test_project_list(prec, C, S, z, B):
    from vae_play_amd import _lib
    vae, inf = _build(prec, C, S, z, B)
    inf.enable_projection()
    L = inf.L
    names = lambda w: [c[0] for p in inf._plans[w] for c in p.calls]      # noqa: E731
    fin = "vp_conv5_smallin_dgrad_bf16x3" if prec == "bf16x3" else "vp_conv5_smallin_dgrad_f32"
    conv = "vp_conv5_gather_bf16x3" if prec == "bf16x3" else "vp_conv5_gather_f32"
    walk = [fin] + L * ["vp_affine_relu_bwd_f32", conv] + ["vp_nhwc_to_nchw_f32", "vp_affine_relu_bwd_f32", "vp_gemm_f32"]
    assert names("project") == names("decode") + ["vp_bce_masked_rows_bwd_f32"] + walk + ["vp_latent_adam_f32"]
    assert names("project.grad") == names("project") and names("project.loss") == names("decode") + ["vp_bce_masked_rows_bwd_f32",
                                                                                                     "vp_latent_adam_f32"]
    new = NEW + (("project.load",) if C > 1 else ())
    assert ("project.load" in inf._plans) == (C > 1) and (C == 1 or names("project.load") == ["vp_nchw_to_nhwc_f32"] * 2)
    # the decode list is the plan's own, not a copy; the objective and the walk are shared by the lists
    assert inf._plans["project"][0] is inf._plans["decode"][0] and inf._plans["project"][1:3] == inf._plans["project.grad"][1:3]
    for w in new:
        for p in inf._plans[w]:
            for c in p.calls:
                assert len(c[2]) == len(_lib.SIGNATURES[c[0]][1]) and c[6] is None, c[0]        # everything on the main stream
    # lifetime: every pointer resolves into _bufs or module tensors after a collection
    gc.collect()
    calls, unknown = _record(vae, inf, new)
    assert unknown == 0, [c[:2] for c in calls if any(isinstance(a, list) and a[:1] == ["?"] for a in c[2])]
    by_name = lambda n, plan: [c for c in calls if c[1] == n and plan in c[0].split("+")]      # noqa: E731
    # one (mask-and-scale, convolution) pair per block, last block first: R x C of the pair grows towards the image
    acts = [c for c in calls if c[1] == "vp_affine_relu_bwd_f32"]
    assert len(acts) == L + 1
    assert [c[4] for c in acts] == [f"dec{i}.dact" for i in reversed(range(L))] + ["dec.fc.dact"]
    dec = inf.decoder
    for c, i in zip(acts[:L], reversed(range(L))):
        Cout = dec.conv[i].conv.weight.shape[1]
        assert c[2][6:8] == [B * (16 << i) ** 2, Cout]
        assert (c[2][1] is None) != (c[2][2] is None) and (c[2][4] is None) != (c[2][5] is None)        # u and dx: fp32 or split, one each
    assert acts[L][2][6:8] == [B, 64 * dec._c0] and acts[L][2][2] is None and acts[L][2][5] is None       # the dense pair is fp32
    # the update: the plan's z, the walk's dz, the defaults of project(), the counter in device memory
    (adam,) = by_name("vp_latent_adam_f32", "project")
    assert adam[2][5:7] == [B, z] and all(a is not None for a in adam[2][:5]) and adam[2][12] is not None
    assert adam[2][7:12] == [float(v).hex() for v in (0.05, 0.9, 0.999, 1e-8, 1.0)]
    gemm = by_name("vp_gemm_f32", "project")[-1]        # (the first is the decode list's dense layer)
    assert gemm[2][6] == adam[2][1]                     # lin_dgrad writes the dz the update reads
    for prior in by_name("vp_latent_adam_f32", "project.grad") + by_name("vp_latent_adam_f32", "project.loss"):
        assert prior[2][0] == adam[2][0] and prior[2][1:5] == [None] * 4 and prior[2][12] == adam[2][12]
    (bce,) = [c for c in calls if c[1] == "vp_bce_masked_rows_bwd_f32"]
    assert bce[2][3:5] == [B, C * S * S] and all(a is not None for a in bce[2][:3] + bce[2][5:8])
    assert bce[2][8] >= _lib.load().vp_bce_masked_rows_bwd_workspace_bytes(B, C * S * S)
    # the projection's own re-pack: the gather-family pack of every block, nothing else
    (pack,) = [c for c in calls if c[0] == "project.prep"]
    assert pack[1] == "vp_pack_w5_batch" and len(pack[2][0]) == L and all(j[1] is not None and j[2] is None for j in pack[2][0])


def test_other_hyperparameters_rebuild_the_tail_only():
    vae, inf = _build("bf16x3", 1, 16, 8, 2)
    inf.enable_projection()
    shared = inf._plans["project"][:3]
    old_tail = inf._plans["project"][3]
    bufs = dict(inf._bufs)
    inf._project_lists(0.01, 0.8, 0.99, 1e-6, 0.5)
    assert inf._plans["project"][:3] == shared and inf._plans["project"][3] is not old_tail
    assert inf._plans["project"][3].calls[0][2][7:12] == [0.01, 0.8, 0.99, 1e-6, 0.5]
    assert inf._plans["project.loss"][2].calls[0][2][11] == 0.5
    assert {n: t.data_ptr() for n, t in inf._bufs.items()} == {n: t.data_ptr() for n, t in bufs.items()}


def test_f16_plans_refuse_projection():
    vae, inf = _build("f16", 3, 32, 16, 2)
    with pytest.raises(NotImplementedError, match="f16"):
        inf.enable_projection()
    assert inf._proj is None and set(inf._plans) == set(OLD) and not any(n.startswith("project") for n in inf._bufs)


def test_projection_refuses_bad_arguments():
    from vae_play_amd import _lib
    vae, inf = _build("bf16x3", 1, 16, 8, 2)
    with pytest.raises(_lib.VaePlayHipError, match="HIP device"):
        inf.project(torch.zeros(2, 1, 16, 16))
    with pytest.raises(_lib.VaePlayHipError, match="HIP device"):
        inf.decode_grad(torch.zeros(2, 8), torch.zeros(2, 1, 16, 16))
    assert inf._proj is None                                # a refused call allocates nothing
