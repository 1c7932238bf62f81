"""SCSEBlock on the device (vae_play_amd/csrc/scse.hip): the reference-generated fixture, an fp64 statement of the formula at the
three StyleUp geometries and at the awkward channel counts, run-to-run bit identity, the fused trailing ReLU, the C ABI's refusals
and two chained blocks.  Everything is held to tests.util.OP_RTOL (max error over max magnitude)."""
from ctypes import c_void_p

import pytest
import torch

from tests.util import OP_RTOL, assert_close, load_golden, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("cSE.1.weight", "cSE.1.bias", "cSE.3.weight", "cSE.3.bias", "sSE.0.weight", "sSE.0.bias")


def scse_fp64(x, params, relu):
    """The block written out: y = x * c + x * s (models/blocks.py:64-65), double precision, plain torch."""
    w1, b1, w2, b2, ws, bs = params
    B, C, H, W = x.shape
    pooled = x.mean(dim=(2, 3))                                               # (B, C)
    hidden = torch.relu(pooled @ w1.reshape(-1, C).t() + b1)                  # (B, C/r)
    c = torch.sigmoid(hidden @ w2.reshape(C, -1).t() + b2)                    # (B, C)     channel gate
    s = torch.sigmoid((x * ws.reshape(1, C, 1, 1)).sum(dim=1, keepdim=True) + bs)     # (B, 1, H, W) spatial gate
    y = x * c.reshape(B, C, 1, 1) + x * s
    return torch.relu(y) if relu else y


def fp64_run(x, dy, params, relu, second=None):
    xd = x.double().requires_grad_(True)
    pd = [p.detach().double().requires_grad_(True) for p in params]
    if second is None:
        y = scse_fp64(xd, pd, relu)
        leaves = pd
    else:
        qd = [p.detach().double().requires_grad_(True) for p in second]
        y = scse_fp64(scse_fp64(xd, pd, False), qd, relu)
        leaves = pd + qd
    y.backward(dy.double())
    return y.detach(), xd.grad, [p.grad for p in leaves]


def make_block(C, r, seed=1, scale=3.0):
    from vae_play_amd.blocks import SCSEBlock
    torch.manual_seed(seed)
    blk = SCSEBlock(C, reduction=r)
    with torch.no_grad():
        for p in blk.parameters():
            p.mul_(scale)                      # gates away from 1/2
    return blk


def params_of(blk):
    sd = dict(blk.named_parameters())
    return [sd[k] for k in KEYS]


def hip_run(blk, x, dy, relu, nchw=False):
    blk = blk.to(DEV)
    blk.zero_grad(set_to_none=True)
    xg = x.to(DEV)
    if not nchw:
        xg = xg.contiguous(memory_format=torch.channels_last)
    xg.requires_grad_(True)
    y = blk(xg, relu=relu) if relu else blk(xg)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    return y.detach().cpu(), xg.grad.cpu(), [p.grad.cpu() for p in params_of(blk)]


def check_against_fp64(B, C, H, W, r, relu, nchw):
    blk = make_block(C, r)
    torch.manual_seed(2)
    x, dy = torch.randn(B, C, H, W), torch.randn(B, C, H, W)
    y_ref, dx_ref, g_ref = fp64_run(x, dy, params_of(blk), relu)
    y, dx, g = hip_run(blk, x, dy, relu, nchw)
    errs = {"y": assert_close(y, y_ref, OP_RTOL, "y"), "dx": assert_close(dx, dx_ref, OP_RTOL, "dx")}
    for k, a, b in zip(KEYS, g, g_ref):
        errs[k] = assert_close(a, b, OP_RTOL, f"grad {k}")
    print(f"scse {B}x{C}x{H}x{W} r{r} relu={relu} nchw={nchw}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))


def test_golden_fixture():
    """Forward and backward of the reference's own class (fp32, CPU) on its seeded parameters."""
    from vae_play_amd.blocks import SCSEBlock
    g = load_golden("blocks_scse_c32_r4")
    blk = SCSEBlock(32, reduction=4)
    blk.load_state_dict({k: t(g[f"state/{k}"]) for k in KEYS}, strict=True)
    y, dx, grads = hip_run(blk, t(g["x"]), t(g["dy"]), False)
    assert_close(y, t(g["y"]), OP_RTOL, "y")
    assert_close(dx, t(g["dx"]), OP_RTOL, "dx")
    for k, a in zip(KEYS, grads):
        assert a.shape == g[f"grad/{k}"].shape, k
        assert_close(a, t(g[f"grad/{k}"]), OP_RTOL, f"grad {k}")


# the three StyleUp stage geometries (batch 2), a channel count that is not a multiple of 4, a one-channel hidden layer, both ReLU
# settings; the 70-channel and the 128-channel case enter as standard-contiguous NCHW tensors
@pytest.mark.parametrize("B,C,H,W,r,relu,nchw", [
    (2, 32, 5, 7, 4, False, False),
    (3, 70, 9, 11, 4, True, True),
    (2, 64, 128, 128, 4, True, False),
    (2, 128, 64, 64, 4, False, True),
    (2, 256, 32, 32, 4, True, False),
    (1, 16, 3, 3, 16, False, False),
])
def test_fp64_statement(B, C, H, W, r, relu, nchw):
    check_against_fp64(B, C, H, W, r, relu, nchw)


# the remaining kernel instantiations and a chunk with a tail: 128 and 256 float4 per pixel (two and four per lane), the scalar path
# with four channels per lane and with eight lanes per pixel, 12 float4 in a 16-lane slot with 1023 pixels in chunks of 170
@pytest.mark.parametrize("B,C,H,W,r,relu", [
    (2, 512, 4, 4, 8, True),
    (1, 1024, 3, 5, 16, False),
    (2, 250, 6, 5, 5, True),
    (2, 6, 17, 13, 2, False),
    (5, 48, 33, 31, 4, True),
])
def test_fp64_statement_other_widths(B, C, H, W, r, relu):
    check_against_fp64(B, C, H, W, r, relu, False)


def test_bit_identical_runs():
    blk = make_block(64, 4)
    torch.manual_seed(2)
    x, dy = torch.randn(4, 64, 48, 40), torch.randn(4, 64, 48, 40)
    for relu in (False, True):
        a = hip_run(blk, x, dy, relu)
        b = hip_run(blk, x, dy, relu)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for k, ga, gb in zip(KEYS, a[2], b[2]):
            assert torch.equal(ga, gb), k


def test_fused_relu_equals_the_composition():
    from vae_play_amd import functional as F_hip
    blk = make_block(128, 4).to(DEV)
    p = params_of(blk)
    torch.manual_seed(2)
    x = torch.randn(3, 128, 20, 24, device=DEV).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(3, 128, 20, 24, device=DEV)
    xa = x.clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    fused = F_hip.scse(xa, *p, relu=True)
    plain = torch.relu(F_hip.scse(xb, *p))
    assert torch.equal(fused, plain)
    assert float((fused == 0).float().mean()) > 0.3, "the ReLU must have something to cut"
    ga = torch.autograd.grad(fused, [xa] + p, dy)
    gb = torch.autograd.grad(plain, [xb] + p, dy)
    for name, a, b in zip(("dx",) + KEYS, ga, gb):
        assert_close(a, b, OP_RTOL, f"fused vs composed {name}")


def test_no_grad_keeps_nothing_and_matches():
    blk = make_block(64, 4).to(DEV)
    torch.manual_seed(2)
    x = torch.randn(2, 64, 16, 16, device=DEV).contiguous(memory_format=torch.channels_last)
    y = blk(x)
    with torch.no_grad():
        z = blk(x)
    assert z.grad_fn is None and not z.requires_grad and torch.equal(y.detach(), z)


def test_abi_refusals():
    from vae_play_amd import _lib
    lib = _lib.load()
    P = lambda a: c_void_p(a.data_ptr())
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    B, HW, C, hid = 2, 35, 32, 8
    f = lambda *shape: torch.randn(*shape, device=DEV)
    x, dy, y, dx = f(B * HW * C), f(B * HW * C), f(B * HW * C), f(B * HW * C)
    w1, b1, w2, b2, ws_, bs = f(hid * C), f(hid), f(C * hid), f(C), f(C), f(1)
    pool, hidden, cg, sg = f(B * C), f(B * hid), f(B * C), f(B * HW)
    need = lib.vp_scse_workspace_bytes(B, HW, C, hid)
    assert need > 64
    wk = torch.empty(need // 4 + 4, device=DEV)
    fwd = lambda h, w, nbytes: lib.vp_scse_fwd_f32(P(x), P(w1), P(b1), P(w2), P(b2), P(ws_), P(bs), P(y), P(pool), P(hidden), P(cg),
                                                   P(sg), B, HW, C, h, 0, w, nbytes, st)
    bwd = lambda h, w, nbytes: lib.vp_scse_bwd_f32(P(x), P(dy), P(w1), P(w2), P(ws_), P(pool), P(hidden), P(cg), P(sg), P(dx), P(w1),
                                                   P(b1), P(w2), P(b2), P(ws_), P(bs), B, HW, C, h, 0, w, nbytes, st)
    # short workspace
    assert fwd(hid, P(wk), need - 64) == -3 and b"workspace" in lib.vp_last_error()
    assert bwd(hid, P(wk), need - 64) == -3 and b"workspace" in lib.vp_last_error()
    # C / reduction == 0: an argument check, nothing is launched
    assert fwd(0, P(wk), need) == -1 and b"C / reduction == 0" in lib.vp_last_error()
    assert bwd(0, P(wk), need) == -1 and b"C / reduction == 0" in lib.vp_last_error()
    # null pointer, non-positive size
    assert fwd(hid, None, need) == -1 and b"null" in lib.vp_last_error()
    assert lib.vp_scse_fwd_f32(P(x), P(w1), P(b1), P(w2), P(b2), P(ws_), P(bs), P(y), P(pool), P(hidden), P(cg), P(sg), B, 0, C, hid, 0,
                               P(wk), need, st) == -1
    # the float4 path needs 16-byte aligned pointers; the scalar path that stands in holds 256 channels, so C = 512 with x one float
    # off an aligned address is refused, not computed on 256 channels of 512
    C5, h5 = 512, 128
    x5, y5, dy5, dx5 = f(B * HW * C5 + 4), f(B * HW * C5 + 4), f(B * HW * C5), f(B * HW * C5)
    v1, c1, v2, c2, vs = f(h5 * C5), f(h5), f(C5 * h5), f(C5), f(C5)
    pool5, hid5, cg5 = f(B * C5), f(B * h5), f(B * C5)
    need5 = lib.vp_scse_workspace_bytes(B, HW, C5, h5)
    wk5 = torch.empty(need5 // 4 + 4, device=DEV)
    fwd5 = lambda xp, yp: lib.vp_scse_fwd_f32(xp, P(v1), P(c1), P(v2), P(c2), P(vs), P(bs), yp, P(pool5), P(hid5), P(cg5), P(sg), B, HW, C5,
                                              h5, 0, P(wk5), need5, st)
    bwd5 = lambda xp, dxp: lib.vp_scse_bwd_f32(xp, P(dy5), P(v1), P(v2), P(vs), P(pool5), P(hid5), P(cg5), P(sg), dxp, P(v1), P(c1), P(v2),
                                               P(c2), P(vs), P(bs), B, HW, C5, h5, 0, P(wk5), need5, st)
    off = lambda a: c_void_p(a.data_ptr() + 4)
    assert x5.data_ptr() % 16 == 0 and y5.data_ptr() % 16 == 0
    assert fwd5(off(x5), P(y5)) == -1 and b"16-byte aligned" in lib.vp_last_error()
    assert fwd5(P(x5), off(y5)) == -1 and b"16-byte aligned" in lib.vp_last_error()
    assert fwd5(P(x5), P(y5)) == 0
    assert bwd5(off(x5), P(dx5)) == -1 and b"16-byte aligned" in lib.vp_last_error()
    assert bwd5(P(x5), P(dx5)) == 0
    # the library is still usable, and the Python wrapper refuses an empty hidden layer too
    assert fwd(hid, P(wk), need) == 0
    torch.cuda.synchronize()
    from vae_play_amd import functional as F_hip
    with pytest.raises(_lib.VaePlayHipError) as e:
        F_hip.scse(torch.randn(1, 8, 4, 4, device=DEV), torch.empty(0, 8, 1, 1, device=DEV), torch.empty(0, device=DEV),
                   torch.empty(8, 0, 1, 1, device=DEV), f(8), f(1, 8, 1, 1), f(1))
    assert "C / reduction == 0" in str(e.value)


def test_unaligned_pointers_take_the_scalar_path():
    """x and y one float off a 16-byte boundary at the C ABI, C = 256 (the widest the scalar path holds): the same function."""
    from vae_play_amd import _lib
    lib = _lib.load()
    B, C, H, W, hid = 2, 256, 5, 7, 64
    blk = make_block(C, 4)
    torch.manual_seed(2)
    x = torch.randn(B, C, H, W)
    y_ref = scse_fp64(x.double(), [p.detach().double() for p in params_of(blk)], True)
    P = lambda a: c_void_p(a.data_ptr())
    n = x.numel()
    xbuf, ybuf = torch.zeros(n + 4, device=DEV), torch.zeros(n + 4, device=DEV)
    xbuf[1:n + 1] = x.permute(0, 2, 3, 1).reshape(-1).to(DEV)
    prm = [p.detach().to(DEV).contiguous() for p in params_of(blk)]
    new = lambda *s: torch.empty(*s, device=DEV)
    pool, hidden, cg, sg = new(B, C), new(B, hid), new(B, C), new(B, H * W)
    need = lib.vp_scse_workspace_bytes(B, H * W, C, hid)
    wk = new(need // 4 + 4)
    assert xbuf.data_ptr() % 16 == 0 and ybuf.data_ptr() % 16 == 0
    rc = lib.vp_scse_fwd_f32(c_void_p(xbuf.data_ptr() + 4), *(P(q) for q in prm), c_void_p(ybuf.data_ptr() + 4), P(pool), P(hidden), P(cg),
                             P(sg), B, H * W, C, hid, 1, P(wk), need, c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.vp_last_error()
    torch.cuda.synchronize()
    y = ybuf[1:n + 1].reshape(B, H, W, C).permute(0, 3, 1, 2).cpu()
    assert_close(y, y_ref, OP_RTOL, "y")
    assert float(ybuf[0]) == 0.0 and float(ybuf[n + 1]) == 0.0, "nothing outside the tensor is written"


def test_fused_relu_keeps_nan():
    """torch.relu hands a NaN on; so does the fused store (every channel of the pixel and, through the mean, of the image)."""
    from vae_play_amd import functional as F_hip
    blk = make_block(32, 4).to(DEV)
    torch.manual_seed(2)
    x = torch.randn(2, 32, 6, 5, device=DEV).contiguous(memory_format=torch.channels_last)
    x[1, 3, 2, 2] = float("nan")
    with torch.no_grad():
        fused = F_hip.scse(x, *params_of(blk), relu=True)
        plain = torch.relu(F_hip.scse(x, *params_of(blk)))
    assert torch.isnan(plain[1]).any() and not torch.isnan(plain[0]).any()
    assert torch.equal(torch.isnan(fused), torch.isnan(plain))
    assert torch.equal(torch.nan_to_num(fused), torch.nan_to_num(plain))


def test_backward_computes_what_is_asked_for():
    """x without requires_grad: no dx is produced and the parameter gradients keep their bits; a parameter without requires_grad
    gets no gradient."""
    blk = make_block(64, 4)
    torch.manual_seed(2)
    x, dy = torch.randn(3, 64, 12, 10), torch.randn(3, 64, 12, 10)
    _, _, g_full = hip_run(blk, x, dy, True)
    blk.zero_grad(set_to_none=True)
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last)
    blk.sSE[0].bias.requires_grad_(False)
    blk(xg, relu=True).backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert xg.grad is None and blk.sSE[0].bias.grad is None
    for k, p, ref in list(zip(KEYS, params_of(blk), g_full))[:-1]:
        assert torch.equal(p.grad.cpu(), ref), k


def test_gradients_land_in_the_arena():
    """Parameters that live in an optimiser's flat arena get their gradients written into their slices (functional._grad_out)."""
    from vae_play_amd.optim import FlatArena
    blk = make_block(32, 4)
    torch.manual_seed(2)
    x, dy = torch.randn(2, 32, 9, 7), torch.randn(2, 32, 9, 7)
    _, dx_ref, g_ref = hip_run(blk, x, dy, False)
    arena = FlatArena(blk.parameters())
    arena.zero_grad(set_to_none=True)
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    blk(xg).backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(xg.grad.cpu(), dx_ref)
    for k, p, ref in zip(KEYS, params_of(blk), g_ref):
        assert p.grad.data_ptr() == arena.grad_view(p).data_ptr(), k
        assert torch.equal(p.grad.cpu(), ref), k


def test_two_blocks_and_relu():
    """The tail of StyleUp.cat_convs (models/network_Style_GAN.py:56-58): SCSE, SCSE, ReLU, the ReLU fused into the second block."""
    B, C, H, W = 2, 64, 24, 40
    b1, b2 = make_block(C, 4, seed=1), make_block(C, 4, seed=3)
    torch.manual_seed(2)
    x, dy = torch.randn(B, C, H, W), torch.randn(B, C, H, W)
    y_ref, dx_ref, g_ref = fp64_run(x, dy, params_of(b1), True, second=params_of(b2))
    b1, b2 = b1.to(DEV), b2.to(DEV)
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = b2(b1(xg), relu=True)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert_close(y, y_ref, OP_RTOL, "y")
    assert_close(xg.grad, dx_ref, OP_RTOL, "dx")
    for (name, p), ref in zip([(f"first {k}", p) for k, p in zip(KEYS, params_of(b1))] +
                              [(f"second {k}", p) for k, p in zip(KEYS, params_of(b2))], g_ref):
        assert_close(p.grad, ref, OP_RTOL, f"grad {name}")
