"""vp_twin_head_{fwd,bwd}_f32 through the C ABI (include/vaeplay_hip.h): the Style-GAN discriminator's output stage against an fp64
statement of its formulas -- F.conv2d(stride 2, padding 1) on the NCHW view of the 2 x 2 maps, sigmoid and softmax, autograd for the
gradients -- held to tests.util.OP_RTOL on NaN-prefilled outputs.  h = randn, weights = randn / sqrt(4C): unit-variance logits, so
that neither the sigmoid nor the softmax saturates and the gradient checks mean something."""
from ctypes import c_void_p

import pytest
import torch
import torch.nn.functional as F

from tests.util import OP_RTOL, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [(3, 256, 2),      # the workload's head: a float4 per lane, all four waves busy
         (2, 32, 3),       # the fixture's head: 32 of 256 lanes hold an element
         (1, 8, 1),        # softmax of one class
         (5, 6, 5),        # C % 4 != 0: the scalar instantiation
         (2, 1024, 64)]    # both limits: four elements per lane, 65 outputs


def P(t):
    return None if t is None else c_void_p(t.data_ptr())


def _inputs(B, C, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    s = (4 * C) ** -0.5
    return dict(h_adv=r(B, 4, C), h_aux=r(B, 4, C), w_adv=r(1, C, 3, 3) * s, b_adv=r(1), w_aux=r(K, C, 3, 3) * s, b_aux=r(K),
                d_adv=r(B, 1), d_aux=r(B, K))


def _reference(i):
    """the fp64 statement: every name of ``_run``'s result"""
    B, _, C = i["h_adv"].shape
    v = {k: t.double().requires_grad_(True) for k, t in i.items() if k[0] in "hwb"}
    nchw = lambda h: h.reshape(B, 2, 2, C).permute(0, 3, 1, 2)
    adv = torch.sigmoid(F.conv2d(nchw(v["h_adv"]), v["w_adv"], v["b_adv"], stride=2, padding=1).reshape(B, -1))
    aux = torch.softmax(F.conv2d(nchw(v["h_aux"]), v["w_aux"], v["b_aux"], stride=2, padding=1).reshape(B, -1), dim=-1)
    torch.autograd.backward([adv, aux], [i["d_adv"].double(), i["d_aux"].double()])
    out = {"adv": adv.detach(), "aux": aux.detach()}
    out.update({"d" + k: t.grad for k, t in v.items()})
    return out


def _run(i, d_adv=True, d_aux=True):
    """forward + backward through the C ABI on NaN-prefilled outputs; ``d_adv`` / ``d_aux`` False passes a null pointer"""
    from vae_play_amd import _lib
    lib = _lib.load()
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    d = {k: t.to(DEV).contiguous() for k, t in i.items()}
    B, _, C = i["h_adv"].shape
    K = i["w_aux"].shape[0]
    nan = lambda like: torch.full_like(like, float("nan"))
    o = {"adv": nan(d["d_adv"]), "aux": nan(d["d_aux"])}
    assert lib.vp_twin_head_fwd_f32(P(d["h_adv"]), P(d["h_aux"]), P(d["w_adv"]), P(d["b_adv"]), P(d["w_aux"]), P(d["b_aux"]), P(o["adv"]),
                                    P(o["aux"]), B, C, K, st) == 0, lib.vp_last_error()
    for k in ("h_adv", "h_aux", "w_adv", "b_adv", "w_aux", "b_aux"):
        o["d" + k] = nan(d[k])
    assert lib.vp_twin_head_bwd_f32(P(d["h_adv"]), P(d["h_aux"]), P(d["w_adv"]), P(d["w_aux"]), P(o["adv"]), P(o["aux"]),
                                    P(d["d_adv"]) if d_adv else None, P(d["d_aux"]) if d_aux else None, P(o["dh_adv"]), P(o["dh_aux"]),
                                    P(o["dw_adv"]), P(o["db_adv"]), P(o["dw_aux"]), P(o["db_aux"]), B, C, K, st) == 0, lib.vp_last_error()
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in o.items()}


_CACHE = {}


def _case(B, C, K):
    """inputs, the kernel's results and the fp64 reference of one case: computed once, shared and left unchanged"""
    if (B, C, K) not in _CACHE:
        i = _inputs(B, C, K)
        _CACHE[B, C, K] = (i, _run(i), _reference(i))
    return _CACHE[B, C, K]


def _live(w):
    return w[:, :, 1:, 1:]


def _dead_bits(dw):
    """the int32 patterns of row 0 and column 0 of every 3x3: all zero means +0.0f bit for bit"""
    m = torch.ones(3, 3, dtype=torch.bool)
    m[1:, 1:] = False
    return dw.view(torch.int32)[:, :, m]


@pytest.mark.parametrize("B,C,K", CASES)
def test_against_fp64(B, C, K):
    _, got, ref = _case(B, C, K)
    errs = {}
    for k in ("adv", "aux", "dh_adv", "dh_aux", "db_adv", "db_aux"):
        assert not torch.isnan(got[k]).any(), f"{k}: an element was not written"
        errs[k] = assert_close(got[k], ref[k].reshape(got[k].shape), OP_RTOL, f"{k} B{B} C{C} K{K}")
    for k in ("dw_adv", "dw_aux"):
        assert not torch.isnan(got[k]).any(), f"{k}: an element was not written"
        errs[k] = assert_close(_live(got[k]), _live(ref[k]), OP_RTOL, f"{k} B{B} C{C} K{K}")
        assert not _dead_bits(got[k]).any(), f"{k}: a tap that only meets padding is not 0.0f"
    print(f"twin head B{B} C{C} K{K}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    if K == 1:      # softmax of one class is the constant 1: nothing flows back
        assert torch.equal(got["aux"], torch.ones(B, 1))
        for k in ("dh_aux", "dw_aux", "db_aux"):
            assert got[k].abs().max().item() == 0.0, k


def test_dead_taps_neither_read_nor_written():
    """1e30 in row 0 and column 0 of every 3x3 weight: same outputs and dh, and dw there stays 0.0f bit for bit"""
    i, got, _ = _case(2, 32, 3)
    j = {k: t.clone() for k, t in i.items()}
    for k in ("w_adv", "w_aux"):
        j[k][:, :, 0, :] = 1e30
        j[k][:, :, :, 0] = 1e30
    big = _run(j)
    for k in ("adv", "aux", "dh_adv", "dh_aux", "db_adv", "db_aux"):
        assert torch.equal(big[k], got[k]), k
    for k in ("dw_adv", "dw_aux"):
        assert torch.equal(_live(big[k]), _live(got[k])), k
        assert not _dead_bits(big[k]).any(), k


def test_null_output_gradient_is_a_zero_gradient():
    i, _, _ = _case(5, 6, 5)
    for null, name in ((dict(d_adv=False), "d_adv"), (dict(d_aux=False), "d_aux")):
        z = {k: (torch.zeros_like(t) if k == name else t) for k, t in i.items()}
        a, b = _run(i, **null), _run(z)
        for k in a:
            assert torch.equal(a[k], b[k]), f"null {name}: {k}"
        side = "adv" if name == "d_adv" else "aux"
        for k in (f"dh_{side}", f"dw_{side}", f"db_{side}"):
            assert a[k].abs().max().item() == 0.0, f"null {name}: {k}"


def test_two_runs_give_the_same_bits():
    i, got, _ = _case(3, 256, 2)
    again = _run(i)
    for k in got:
        assert torch.equal(again[k].view(torch.int32), got[k].view(torch.int32)), k


def test_refusals():
    """arguments outside the stated range and a null required pointer: VP_ERR_ARG, nothing launched, the library stays usable"""
    from vae_play_amd import _lib
    lib = _lib.load()
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    h = torch.randn(2, 4, 8, device=DEV)
    w = torch.randn(2, 8, 3, 3, device=DEV)
    b = torch.randn(2, device=DEV)
    o = torch.full((2, 2), float("nan"), device=DEV)
    big = torch.empty(1, device=DEV)        # never read: the calls below are refused before anything is launched
    fwd = lambda ha, C, K: lib.vp_twin_head_fwd_f32(ha, P(h), P(w), P(b), P(w), P(b), P(o), P(o), 2, C, K, st)
    bwd = lambda ha, C, K: lib.vp_twin_head_bwd_f32(ha, P(h), P(w), P(w), P(o), P(o), P(o), P(o), P(big), P(big), P(big), P(big), P(big),
                                                    P(big), 2, C, K, st)
    for call in (fwd, bwd):
        assert call(P(h), 8, 0) == -1 and b"K = 0" in lib.vp_last_error()
        assert call(P(h), 8, 65) == -1 and b"K = 65" in lib.vp_last_error()
        assert call(P(h), 1025, 2) == -1 and b"C = 1025" in lib.vp_last_error()
        assert call(None, 8, 2) == -1 and b"null" in lib.vp_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(o).all(), "a refused call wrote"
    i, got, _ = _case(1, 8, 1)
    assert torch.equal(_run(i)["adv"], got["adv"])
