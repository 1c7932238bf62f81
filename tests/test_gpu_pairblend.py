"""vp_pair_blend_{fwd,bwd}_f32: the normalise-and-blend pass behind the stacked convolution of a label-gated pair
(models/network_Style_GAN.py:72-79), y = (1 - label) * act(n(u_1)) + label * act(n(u_2)), through the C ABI against the fp64 torch
formula (autograd supplies du).  Tolerance tests/util.OP_RTOL, relative to the tensor's max.

ReLU cases draw u so that every normalised value keeps |u^| >= 1e-4 (checked on the CPU in fp64 before anything is launched; the
next seed is taken otherwise): fp32 rounds u^ to about 1e-6, so no mask can differ between the kernel and the formula."""
from ctypes import c_void_p

import pytest
import torch

from tests.util import OP_RTOL, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
ACT = {"none": 0, "relu": 1}
# (B, R, C): small vector path | down4 at image size 32 | three reduction chunks with a ragged last one (48, 48, 47 rows of 143 under
# bn.hip's bn_grid for 2C = 32) | scalar tail path (C % 4 != 0, no split planes)
SHAPES = [(3, 35, 8), (2, 4, 256), (2, 143, 16), (2, 35, 6)]


def P(t):
    return None if t is None else c_void_p(t.data_ptr())


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _labels(B):
    return torch.tensor([(0.0, 1.0, 0.25)[b % 3] for b in range(B)])


def _formula(u, dy, label, norm, act):
    """fp64: (y, du, u^, mean, rstd) for u (B, R, 2C), dy (B, R, C), label (B,)"""
    u = u.double().requires_grad_(True)
    C = u.shape[2] // 2
    mean = u.mean(1, keepdim=True)
    rstd = (u.var(1, unbiased=False, keepdim=True) + EPS).rsqrt()
    uh = (u - mean) * rstd if norm else u
    a = torch.relu(uh) if act == "relu" else uh
    w2 = label.double().reshape(-1, 1, 1)
    y = (1 - w2) * a[..., :C] + w2 * a[..., C:]
    y.backward(dy.double())
    return y.detach(), u.grad, uh.detach(), mean.detach()[:, 0], rstd.detach()[:, 0]


def _draw(B, R, C, norm, act):
    for seed in range(1000 * B + R + C, 1000 * B + R + C + 64):
        g = torch.Generator().manual_seed(seed)
        u = torch.randn(B, R, 2 * C, generator=g) * 1.5 + 0.3
        dy = torch.randn(B, R, C, generator=g)
        ref = _formula(u, dy, _labels(B), norm, act)
        if act != "relu" or ref[2].abs().min().item() >= 1e-4:
            return u, dy, ref
    raise AssertionError("no draw keeps the ReLU margin")


NAN16 = 0x7FC0       # bf16 NaN in both planes


def _run(lib, u, dy, label, norm, act, split):
    """both entry points on NaN-filled outputs; returns (y, mean, rstd, ys, du, dus)"""
    from vae_play_amd import _lib
    B, R, C2 = u.shape
    C = C2 // 2
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    y, du = nan(B, R, C), nan(B, R, C2)
    mean, rstd = (nan(B, C2), nan(B, C2)) if norm else (None, None)
    ys = torch.full((2, B * R * C), NAN16, dtype=torch.int16, device=DEV) if split else None
    dus = torch.full((2, B * R * C2), NAN16, dtype=torch.int16, device=DEV) if split else None
    nb = lib.vp_pair_blend_workspace_bytes(B, R, C)
    ws = torch.empty(nb // 4 + 1, device=DEV) if norm else None
    _lib.call("vp_pair_blend_fwd_f32", P(u), P(label), P(y), P(ys), P(mean), P(rstd), B, R, C, norm, EPS, ACT[act], 0.0, P(ws),
              nb if norm else 0, _stream())
    _lib.call("vp_pair_blend_bwd_f32", P(u), P(dy), P(label), P(mean), P(rstd), P(du), P(dus), B, R, C, norm, ACT[act], 0.0, P(ws),
              nb if norm else 0, _stream())
    torch.cuda.synchronize()
    return y, mean, rstd, ys, du, dus


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("B,R,C", SHAPES)
def test_pair_blend_against_fp64_formula(B, R, C, norm, act):
    from vae_play_amd import _lib, ops
    lib = _lib.load()
    u_c, dy_c, (y64, du64, _, mean64, rstd64) = _draw(B, R, C, norm, act)
    u, dy, label = u_c.to(DEV), dy_c.to(DEV), _labels(B).to(DEV)
    split = C % 4 == 0
    y, mean, rstd, ys, du, dus = _run(lib, u, dy, label, norm, act, split)
    for name, v in (("y", y), ("du", du), ("mean", mean), ("rstd", rstd)):
        assert v is None or not torch.isnan(v).any(), f"{name}: elements never written"
    tag = f"{(B, R, C)} norm={norm} {act}"
    errs = {"y": assert_close(y, y64, OP_RTOL, f"y {tag}"), "du": assert_close(du, du64, OP_RTOL, f"du {tag}")}
    if norm:
        errs["mean"] = assert_close(mean, mean64, OP_RTOL, f"mean {tag}")
        errs["rstd"] = assert_close(rstd, rstd64, OP_RTOL, f"rstd {tag}")
    print(f"pair_blend {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    # split planes: hi + lo reconstructs the fp32 value to 2^-16 relative, element by element
    if split:
        for name, planes, v in (("y", ys, y), ("du", dus, du)):
            back = ops.unsplit(planes).reshape(v.shape)
            assert not torch.isnan(back).any(), f"{name} planes: elements never written"
            assert ((back - v).abs() <= 2.0 ** -16 * v.abs()).all(), f"{name} planes do not reconstruct the fp32 value"
    # a label of exactly 0 or 1 selects one branch: y is that half's InstanceNorm + activation, the other half gets no gradient
    for b in range(B):
        lab = label[b].item()
        if lab not in (0.0, 1.0):
            continue
        sel, other = (slice(C, 2 * C), slice(0, C)) if lab == 1.0 else (slice(0, C), slice(C, 2 * C))
        assert (du[b, :, other] == 0).all(), f"image {b}: the unselected half of du is not exactly zero"
        if norm:
            half = u[b:b + 1, :, sel].contiguous()
            yh, mh, rh = torch.empty_like(half), torch.empty(1, C, device=DEV), torch.empty(1, C, device=DEV)
            nb = lib.vp_instnorm_workspace_bytes(1, R, C)
            ws = torch.empty(nb // 4 + 1, device=DEV)
            _lib.call("vp_instnorm_act_fwd_f32", P(half), P(yh), P(mh), P(rh), 1, R, C, EPS, ACT[act], 0.0, P(ws), nb, _stream())
            assert_close(y[b:b + 1], yh, OP_RTOL, f"y of image {b} against vp_instnorm_act_fwd_f32 {tag}")
    # fixed-order reductions: a second run gives the same bits
    again = _run(lib, u, dy, label, norm, act, split)
    for name, a, b_ in zip(("y", "mean", "rstd", "ys", "du", "dus"), (y, mean, rstd, ys, du, dus), again):
        assert a is None or torch.equal(a, b_), f"{name}: two runs differ"


def test_pair_blend_error_returns():
    from vae_play_amd import _lib
    lib = _lib.load()
    st = _stream()
    B, R, C = 2, 35, 8
    u, dy, label = torch.randn(B, R, 2 * C, device=DEV), torch.randn(B, R, C, device=DEV), _labels(B).to(DEV)
    y, du = torch.empty(B, R, C, device=DEV), torch.empty(B, R, 2 * C, device=DEV)
    mean, rstd = torch.empty(B, 2 * C, device=DEV), torch.empty(B, 2 * C, device=DEV)
    nb = lib.vp_pair_blend_workspace_bytes(B, R, C)
    assert nb >= lib.vp_instnorm_workspace_bytes(B, R, 2 * C) > 0
    ws = torch.empty(nb // 4 + 1, device=DEV)
    fwd = lambda **k: lib.vp_pair_blend_fwd_f32(P(k.get("u", u)), P(k.get("label", label)), P(k.get("y", y)), P(k.get("ys")),
                                                P(k.get("mean", mean)), P(rstd), B, R, k.get("C", C), 1, EPS, 1, 0.0, P(ws),
                                                k.get("nb", nb), st)
    bwd = lambda **k: lib.vp_pair_blend_bwd_f32(P(k.get("u", u)), P(k.get("dy", dy)), P(label), P(k.get("mean", mean)), P(rstd),
                                                P(k.get("du", du)), P(k.get("dus")), B, R, k.get("C", C), 1, 1, 0.0, P(ws), k.get("nb", nb), st)
    # null pointers
    for call, name, nulls in ((fwd, b"vp_pair_blend_fwd_f32", ("u", "label", "y", "mean")), (bwd, b"vp_pair_blend_bwd_f32", ("u", "dy", "du", "mean"))):
        for n in nulls:
            assert call(**{n: None}) == -1 and name in lib.vp_last_error(), (name, n)
    # split planes need C % 4 == 0 (C = 6 fits inside the buffers allocated for C = 8)
    planes = torch.empty((2, B * R * 2 * C), dtype=torch.int16, device=DEV)
    assert fwd(C=6, ys=planes) == -1 and b"vp_pair_blend_fwd_f32" in lib.vp_last_error() and b"multiple of 4" in lib.vp_last_error()
    assert bwd(C=6, dus=planes) == -1 and b"vp_pair_blend_bwd_f32" in lib.vp_last_error() and b"multiple of 4" in lib.vp_last_error()
    # short workspace -> VP_ERR_WORKSPACE
    assert fwd(nb=nb - 4) == -3 and b"vp_pair_blend_fwd_f32: workspace" in lib.vp_last_error()
    assert bwd(nb=nb - 4) == -3 and b"vp_pair_blend_bwd_f32: workspace" in lib.vp_last_error()
    # and the library stays usable
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
