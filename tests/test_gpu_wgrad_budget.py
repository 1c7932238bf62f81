"""The weight-gradient entry points with a CU budget (vp_conv5_wgrad_{f32,bf16x3,f16x2}_cus) at the benchmark shard's layers, called
directly: with EXACTLY the queried workspace followed by a guard region of the same size, and a guard tail behind dW, both filled with
a bit pattern that must survive every budget -- including budgets above the chip's 256 CUs, which behave as 256 (the workspace query
sizes the row-of-taps slabs for 256 work items).  The results must meet the fp64 direct sum (tests/conv_ref.py) within the tolerance
of their arithmetic, repeat bit for bit, and equal the plain entry point at max_cus = 0.  The other weight-gradient entry points of the
fused step get the same guard check once at their step shapes."""
import pytest
import torch

from tests import conv_ref
from tests.test_gpu_properties import GSCALE, TAU, _layers

pytestmark = pytest.mark.gpu
DEV = "cuda"

B = 32
LAYERS = _layers(128, 4)                # the benchmark shard: bn = 64 and 128, Ws = 8, 16, 32, 64
BUDGETS = (0, 1, 96, 160, 256, 512)
PATTERN = 0x5A5AA5A5


def _guarded(n):
    """n floats followed by n guard floats, all set to PATTERN"""
    buf = torch.empty(2 * max(n, 1), device=DEV)
    buf.view(torch.int32).fill_(PATTERN)
    return buf


def _intact(guard):
    return bool((guard.view(torch.int32) == PATTERN).all().item())


def _call_guarded(lib, fn, lead, tail, nbytes, n_out):
    """fn(*lead, dw, *tail, ws, nbytes, stream) with guarded buffers; returns dW (flat copy)"""
    from vae_play_amd import ops
    assert nbytes > 0 and nbytes % 4 == 0
    nws = nbytes // 4
    ws, dwb = _guarded(nws), _guarded(n_out)
    rc = getattr(lib, fn)(*lead, ops._p(dwb), *tail, ops._p(ws), nbytes, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"{fn} returned {rc}"
    assert _intact(ws[nws:]), f"{fn} wrote past its queried workspace of {nbytes} bytes"
    assert _intact(dwb[n_out:]), f"{fn} wrote past dW"
    return dwb[:n_out].clone()


@pytest.mark.parametrize("name,Cb,Cs,Hs", LAYERS, ids=[ly[0] for ly in LAYERS])
@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f16x2"])
def test_wgrad_cu_budget_stays_in_the_queried_workspace(name, Cb, Cs, Hs, precision):
    from vae_play_amd import _lib, ops
    lib = _lib.load()
    Hb = 2 * Hs
    gen = torch.Generator(device=DEV).manual_seed(sum(map(ord, name + precision)))
    x = torch.randn(B, Hb, Hb, Cb, device=DEV, generator=gen).permute(0, 3, 1, 2)
    y = torch.randn(B, Hs, Hs, Cs, device=DEV, generator=gen).permute(0, 3, 1, 2)
    if precision == "f32":
        nbytes = lib.vp_conv5_wgrad_workspace_bytes(B, Hs, Hs, Cb, Cs, 2)
        lead, scale, tau = (ops._p(x), ops._p(y)), (), TAU["f32"]
    elif precision == "bf16x3":
        nbytes = lib.vp_conv5_wgrad_bf16x3_workspace_bytes(B, Hs, Hs, Cb, Cs, 2)
        xs, ys = ops.split_f32(x), ops.split_f32(y)
        lead, scale, tau = (ops._pv(xs), ops._pv(ys)), (), TAU["bf16x3"]
    else:
        nbytes = lib.vp_conv5_wgrad_bf16x3_workspace_bytes(B, Hs, Hs, Cb, Cs, 2)
        xs, ys = ops.split_f32(x, ops.SPLIT_F16), ops.split_f32(y, ops.SPLIT_F16, GSCALE)
        lead, scale, tau = (ops._pv(xs), ops._pv(ys)), (1.0 / GSCALE,), TAU["f16x2/2"]
    fn = f"vp_conv5_wgrad_{precision}"
    geom = (B, Hs, Hs, Cb, Cs, 2)
    n_out = Cs * Cb * 25
    cs, cb = conv_ref.edge_channels(Cs), conv_ref.edge_channels(Cb)
    r, A = conv_ref.wgrad_ref(x, y, cs, cb)
    res = {}
    for cus in BUDGETS:
        dw = _call_guarded(lib, fn + "_cus", lead, geom + scale + (cus,), nbytes, n_out)
        again = _call_guarded(lib, fn + "_cus", lead, geom + scale + (cus,), nbytes, n_out)
        assert torch.equal(dw, again), f"{name} {precision} max_cus={cus}: two calls differ"
        err, i = conv_ref.worst(dw.view(Cs, Cb, 5, 5)[cs][:, cb], r, A)
        assert err <= tau, f"{name} {precision} max_cus={cus}: |dW - r| = {err:.2e} * A > tau {tau:.0e} (sample {i})"
        res[cus] = dw
    assert torch.equal(res[512], res[256]), f"{name} {precision}: max_cus = 512 must behave as 256"
    plain = _call_guarded(lib, fn, lead, geom + scale, nbytes, n_out)
    assert torch.equal(res[0], plain), f"{name} {precision}: max_cus = 0 must equal the plain entry point"


STEP_ENTRIES = ["vp_conv_wgrad_f32", "vp_conv_wgrad_bf16x3", "vp_conv_wgrad_f16x2",
                "vp_conv5_smallout_wgrad_bf16x3", "vp_conv5_smallout_wgrad_f32"]


@pytest.mark.parametrize("fn", STEP_ENTRIES)
def test_step_wgrad_entry_points_stay_in_the_queried_workspace(fn):
    """The first encoder conv's 1x1 form on its im2col planes (128 px: 64 x 64 outputs, 3 image channels -> 64) and the final conv's
    weight gradient (64 -> 3 channels at 128 x 128), at the benchmark's 32 images: guards intact, and dW against an fp64 sum."""
    from vae_play_amd import _lib, ops
    lib = _lib.load()
    gen = torch.Generator(device=DEV).manual_seed(sum(map(ord, fn)))
    if fn.startswith("vp_conv_wgrad"):
        Hs, Cs = 64, 64
        KC = lib.vp_im2col5s2_cols(3)
        big = torch.randn(B * Hs * Hs, KC, device=DEV, generator=gen)
        small = torch.randn(B * Hs * Hs, Cs, device=DEV, generator=gen)
        geom = (B, Hs, Hs, Hs, Hs, KC, Cs, 1, 1)
        if fn.endswith("f32"):
            nbytes = lib.vp_conv_wgrad_workspace_bytes(*geom)
            lead, tail, tau = (ops._p(big), ops._p(small)), geom, TAU["f32"]
        elif fn.endswith("bf16x3"):
            nbytes = lib.vp_conv_wgrad_bf16x3_workspace_bytes(*geom)
            bs, ss = ops.split_f32(big), ops.split_f32(small)
            lead, tail, tau = (ops._pv(bs), ops._pv(ss)), geom, TAU["bf16x3"]
        else:
            nbytes = lib.vp_conv_wgrad_bf16x3_workspace_bytes(*geom)
            bs, ss = ops.split_f32(big, ops.SPLIT_F16), ops.split_f32(small, ops.SPLIT_F16, GSCALE)
            lead, tail, tau = (ops._pv(bs), ops._pv(ss)), geom + (1.0 / GSCALE,), TAU["f16x2/2"]
        dw = _call_guarded(lib, fn, lead, tail, nbytes, Cs * KC).view(Cs, KC)
        r = small.double().t() @ big.double()
        A = small.double().abs().t() @ big.double().abs()
    else:
        H, Cb, Cs = 128, 64, 3
        big = torch.randn(B, H, H, Cb, device=DEV, generator=gen)
        small = torch.randn(B, H, H, Cs, device=DEV, generator=gen)
        nbytes = getattr(lib, fn + "_workspace_bytes")(B, H, H, Cb, Cs)
        tau = TAU["f32" if fn.endswith("f32") else "bf16x3"]
        dw = _call_guarded(lib, fn, (ops._p(big), ops._p(small)), (B, H, H, Cb, Cs), nbytes, Cs * Cb * 25).view(Cs, Cb, 5, 5)
        # stride 1, padding 2: dW[c, k, r, q] = sum_{b, h, w} small[b, h, w, c] * big[b, h + r - 2, w + q - 2, k]
        s = small.double()
        g = torch.nn.functional.pad(big.double(), (0, 0, 2, 2, 2, 2))
        r = torch.empty(Cs, Cb, 5, 5, dtype=torch.float64, device=DEV)
        A = torch.empty_like(r)
        for i in range(5):
            for j in range(5):
                t = g[:, i:i + H, j:j + H, :]
                r[:, :, i, j] = torch.einsum("bhwc,bhwk->ck", s, t)
                A[:, :, i, j] = torch.einsum("bhwc,bhwk->ck", s.abs(), t.abs())
    err, i = conv_ref.worst(dw, r, A)
    assert err <= tau, f"{fn}: |dW - r| = {err:.2e} * A > tau {tau:.0e} (element {i})"
