"""Tensor-level wrappers over the C ABI (one function per entry point of include/vaeplay_hip.h).

Conventions: activations are 4-D tensors with *logical* NCHW shape stored channels_last
(= NHWC in memory, what the kernels index), or 2-D [R, C] matrices; everything is fp32 on
the current HIP device and stream.  These wrappers only marshal pointers -- all arithmetic
happens in libvaeplay_hip.so.
"""
from __future__ import annotations

from ctypes import c_void_p
from typing import Optional, Tuple

import torch

from . import _lib

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
ACT_CODES = {None: ACT_NONE, "none": ACT_NONE, "relu": ACT_RELU, "lrelu": ACT_LRELU, "tanh": ACT_TANH,
             "sigmoid": ACT_SIGMOID}


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.VaePlayHipError("vae_play_amd ops need tensors on the HIP device (no CPU path exists)")
    if t.dtype != torch.float32:
        raise _lib.VaePlayHipError(f"fp32 tensor expected, got {t.dtype}")
    return c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


CAPTURE_OK = [False]     # set by the fused plans (engine.FusedVAEStep.capture) around their own hipGraph capture


def _stream():
    """The current HIP stream of the current device as a raw pointer.  torch.cuda.current_stream() builds a Stream object per call
    (13 % of the host time of a launch-bound autograd step); torch's raw-stream accessor is one C call.

    hipGraph capture of the AUTOGRAD front end is refused here, before anything is launched into the capture: autograd's
    AccumulateGrad nodes live on the stream their parameters were first used on (normally the default stream), the engine
    synchronises that stream with the capturing one -- illegal inside a capture -- and every launch after that returns
    "capture invalidated" on an autograd worker thread, which ends the process (round 2: gpurun_out/be_graph.err, a core dump
    right after torch's AccumulateGrad-stream warning).  The pre-planned steps (engine.FusedVAEStep / engine_gan.FusedVAEGANStep)
    are the graph-capturable front ends.  The check costs nothing on the default stream (raw handle 0), where no capture can run."""
    if _raw_stream is not None:
        h = _raw_stream(torch.cuda.current_device())
        if h and not CAPTURE_OK[0] and torch.cuda.is_current_stream_capturing():
            raise _lib.VaePlayHipError(
                "hipGraph capture of the autograd front end is not supported (autograd's AccumulateGrad nodes synchronise with "
                "the stream their parameters were first used on, which invalidates the capture and aborts the process); "
                "capture engine.FusedVAEStep / engine_gan.FusedVAEGANStep instead, or run this step eagerly")
        return c_void_p(h)
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws(nbytes: int, like: torch.Tensor) -> torch.Tensor:
    return torch.empty(max(4, (nbytes + 3) // 4), dtype=torch.float32, device=like.device)


def channels_last(x: torch.Tensor) -> torch.Tensor:
    """Logical NCHW tensor whose memory is NHWC: no copy when it already is, the HIP transpose
    for a standard-contiguous NCHW tensor, torch's strided copy only for exotic strides."""
    if x.is_contiguous(memory_format=torch.channels_last):
        return x
    if x.is_contiguous() and x.is_cuda and x.dtype == torch.float32:
        return nchw_to_nhwc(x)
    return x.contiguous(memory_format=torch.channels_last)


def empty_cl(B: int, C: int, H: int, W: int, like: torch.Tensor) -> torch.Tensor:
    return torch.empty((B, C, H, W), dtype=torch.float32, device=like.device, memory_format=torch.channels_last)


def _same_layout(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same shape and same memory order (strides of size-1 dims are irrelevant)."""
    if a.shape != b.shape:
        return False
    return all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n > 1)


def _is_nhwc(x: torch.Tensor) -> bool:
    return x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)


# ---- layout --------------------------------------------------------------------------------
def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    """Copy a standard-contiguous NCHW tensor into a channels_last one with the HIP transpose."""
    B, C, H, W = x.shape
    x = x.contiguous()
    out = empty_cl(B, C, H, W, x)
    _lib.call("vp_nchw_to_nhwc_f32", _p(x), _p(out), B, C, H, W, _stream())
    return out


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    B, C, H, W = x.shape
    assert _is_nhwc(x)
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    _lib.call("vp_nhwc_to_nchw_f32", _p(x), _p(out), B, C, H, W, _stream())
    return out


def pack_w5(w_ref: torch.Tensor, want_p0: bool, want_p1: bool) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """w_ref [Cs][Cb][5][5] -> p0 [Cs][25][Cb], p1 [Cb][25][Cs]."""
    Cs, Cb = w_ref.shape[0], w_ref.shape[1]
    assert w_ref.shape[2:] == (5, 5)
    w_ref = w_ref.contiguous()
    p0 = torch.empty((Cs, 25, Cb), dtype=torch.float32, device=w_ref.device) if want_p0 else None
    p1 = torch.empty((Cb, 25, Cs), dtype=torch.float32, device=w_ref.device) if want_p1 else None
    _lib.call("vp_pack_w5_f32", _p(w_ref), _p(p0), _p(p1), Cs, Cb, _stream())
    return p0, p1


# ---- 5x5 convolution families ----------------------------------------------------------------
def conv5_gather(big: torch.Tensor, w_p0: torch.Tensor, bias: Optional[torch.Tensor], stride: int,
                 act: int = ACT_NONE) -> torch.Tensor:
    """small = act(bias + conv5x5_pad2_stride(big)); big is (B,Cb,Hb,Wb) channels_last."""
    assert _is_nhwc(big)
    B, Cb, Hb, Wb = big.shape
    Cs = w_p0.shape[0]
    assert w_p0.shape == (Cs, 25, Cb) and Hb % stride == 0 and Wb % stride == 0
    Hs, Ws = Hb // stride, Wb // stride
    out = empty_cl(B, Cs, Hs, Ws, big)
    _lib.call("vp_conv5_gather_f32", _p(big), _p(w_p0), _p(bias), _p(out), B, Hs, Ws, Cb, Cs, stride, act, _stream())
    return out


def conv5_scatter(small: torch.Tensor, w_p1: torch.Tensor, stride: int) -> torch.Tensor:
    """big = convT5x5_pad2_stride(small) (output_padding = stride-1); small is (B,Cs,Hs,Ws) channels_last."""
    assert _is_nhwc(small)
    B, Cs, Hs, Ws = small.shape
    Cb = w_p1.shape[0]
    assert w_p1.shape == (Cb, 25, Cs)
    out = empty_cl(B, Cb, Hs * stride, Ws * stride, small)
    _lib.call("vp_conv5_scatter_f32", _p(small), _p(w_p1), _p(out), B, Hs, Ws, Cs, Cb, stride, _stream())
    return out


def _out(out: Optional[torch.Tensor], shape, device) -> torch.Tensor:
    """``out`` (a caller-owned fp32 buffer of that shape, e.g. a parameter's slice of the optimiser's gradient arena) or a new tensor"""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    assert tuple(out.shape) == tuple(shape) and out.is_contiguous() and out.dtype == torch.float32
    return out


def conv5_wgrad(big: torch.Tensor, small: torch.Tensor, stride: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW[Cs][Cb][5][5] in the reference layout."""
    assert _is_nhwc(big) and _is_nhwc(small)
    B, Cb, Hb, Wb = big.shape
    _, Cs, Hs, Ws = small.shape
    assert Hb == Hs * stride and Wb == Ws * stride and small.shape[0] == B
    nbytes = _lib.load().vp_conv5_wgrad_workspace_bytes(B, Hs, Ws, Cb, Cs, stride)
    ws = _ws(nbytes, big)
    dw = _out(out, (Cs, Cb, 5, 5), big.device)
    _lib.call("vp_conv5_wgrad_f32", _p(big), _p(small), _p(dw), B, Hs, Ws, Cb, Cs, stride, _p(ws), ws.numel() * 4, _stream())
    return dw


# ---- dense ------------------------------------------------------------------------------------
def gemm(A: torch.Tensor, sam: int, sak: int, Bm: torch.Tensor, sbn: int, sbk: int, M: int, N: int, K: int, mode: int,
         bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    nbytes = _lib.load().vp_gemm_workspace_bytes(M, N, K)
    ws = _ws(nbytes, A) if nbytes else None
    _lib.call("vp_gemm_f32", _p(A), sam, sak, _p(Bm), sbn, sbk, _p(out), out.stride(0), _p(bias), M, N, K, mode,
              _p(ws), (ws.numel() * 4 if ws is not None else 0), _stream())
    return out


def linear_fwd(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """y[M,N] = x[M,K] W[N,K]^T + bias."""
    x, W = x.contiguous(), W.contiguous()
    M, K = x.shape
    N = W.shape[0]
    return gemm(x, K, 1, W, K, 1, M, N, K, 0, bias)


def linear_dgrad(dy: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """dx[M,K] = dy[M,N] W[N,K]."""
    dy, W = dy.contiguous(), W.contiguous()
    M, N = dy.shape
    K = W.shape[1]
    return gemm(dy, N, 1, W, 1, K, M, K, N, 1)


def linear_wgrad(dy: torch.Tensor, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW[N,K] = dy[M,N]^T x[M,K]."""
    dy, x = dy.contiguous(), x.contiguous()
    M, N = dy.shape
    K = x.shape[1]
    return gemm(dy, 1, N, x, 1, K, N, K, M, 2, out=out)


def conv3_small_wgrad_applicable(B: int, H: int, W: int, Cin: int, Cout: int) -> bool:
    return _lib.load().vp_conv3_small_wgrad_workspace_bytes(B, H, W, Cin, Cout) > 0


def conv3_small_wgrad(x: torch.Tensor, dy: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW (Cout, Cin, 3, 3) of a 3x3 / stride 1 / padding 1 convolution with few channels; x, dy: (B, C, H, W) channels_last fp32."""
    B, Ci, H, W = x.shape
    Co = dy.shape[1]
    assert _is_nhwc(x) and _is_nhwc(dy) and tuple(dy.shape) == (B, Co, H, W)
    nbytes = _lib.load().vp_conv3_small_wgrad_workspace_bytes(B, H, W, Ci, Co)
    if nbytes == 0:
        raise _lib.VaePlayHipError("vp_conv3_small_wgrad_f32 does not take this shape")
    ws = _ws(nbytes, x)
    dw = _out(out, (Co, Ci, 3, 3), x.device)
    _lib.call("vp_conv3_small_wgrad_f32", _p(x), _p(dy), _p(dw), B, H, W, Ci, Co, _p(ws), ws.numel() * 4, _stream())
    return dw


def conv3_small_fwd(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """y = bias + conv3x3(x) (stride 1, padding 1) for few channels; x (B, Ci, H, W) channels_last, weight (Co, Ci, 3, 3)."""
    B, Ci, H, W = x.shape
    Co = weight.shape[0]
    assert _is_nhwc(x) and weight.is_contiguous()
    y = empty_cl(B, Co, H, W, x)
    _lib.call("vp_conv3_small_fwd_f32", _p(x), _p(weight), _p(bias), _p(y), B, H, W, Ci, Co, _stream())
    return y


def conv3_small_dgrad(dy: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    B, Co, H, W = dy.shape
    Ci = weight.shape[1]
    assert _is_nhwc(dy) and weight.is_contiguous()
    dx = empty_cl(B, Ci, H, W, dy)
    _lib.call("vp_conv3_small_dgrad_f32", _p(dy), _p(weight), _p(dx), B, H, W, Ci, Co, _stream())
    return dx


def wgrad_slab_reduce(slab: torch.Tensor, Cs: int, Cb: int, nt: int, variant: int = -1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """slab[nsplit][nt][Cs][Cb] (the K-split weight-gradient launches' workspace) -> dw[Cs][Cb][nt], splits summed in a fixed order."""
    nsplit = slab.numel() // (nt * Cs * Cb)
    assert slab.is_contiguous() and slab.numel() == nsplit * nt * Cs * Cb
    if out is None:
        out = torch.empty((Cs, Cb, nt), device=slab.device, dtype=torch.float32)
    _lib.call("vp_wgrad_slab_reduce_f32", _p(slab), _p(out), Cs, Cb, nsplit, nt, variant, _stream())
    return out


def colsum(x2d: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    R, C = x2d.shape
    assert x2d.is_contiguous()
    ws = _ws(_lib.load().vp_colsum_workspace_bytes(R, C), x2d)
    out = _out(out, (C,), x2d.device)
    _lib.call("vp_colsum_f32", _p(x2d), _p(out), R, C, _p(ws), ws.numel() * 4, _stream())
    return out


# ---- BatchNorm + activation over an [R][C] view ---------------------------------------------------
def _rc(x: torch.Tensor) -> Tuple[int, int]:
    if x.dim() == 2:
        assert x.is_contiguous()
        return x.shape[0], x.shape[1]
    assert _is_nhwc(x)
    B, C, H, W = x.shape
    return B * H * W, C


def bn_stats(x, eps, momentum, running_mean=None, running_var=None):
    R, C = _rc(x)
    mean = torch.empty((C,), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    ws = _ws(_lib.load().vp_bn_workspace_bytes(R, C), x)
    _lib.call("vp_bn_stats_f32", _p(x), R, C, float(eps), float(momentum), _p(mean), _p(rstd), _p(running_mean),
              _p(running_var), _p(ws), ws.numel() * 4, _stream())
    return mean, rstd


def bn_act_fwd(x, mean, rstd, gamma, beta, act: int, slope: float = 0.0, want_split: bool = False):
    """``want_split``: also emit the bf16 hi/lo planes of y from the same pass (C % 4 == 0); returns (y, y_split)."""
    R, C = _rc(x)
    y = torch.empty_like(x)  # preserves channels_last strides
    if want_split:
        ys = empty_split(x.numel(), x)
        _lib.call("vp_bn_act_fwd_split_f32", _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(y), _pv(ys), R, C, act, float(slope),
                  _stream())
        return y, ys
    _lib.call("vp_bn_act_fwd_f32", _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(y), R, C, act, float(slope), _stream())
    return y


def bn_act_bwd(x, dy, mean, rstd, gamma, beta, act: int, slope: float, batch_stats: bool, need_affine_grads: bool = True,
               out_dgamma: Optional[torch.Tensor] = None, out_dbeta: Optional[torch.Tensor] = None, want_split: bool = False):
    """``want_split``: also emit the bf16 hi/lo planes of dx from the same pass (C % 4 == 0); returns (dx, dgamma, dbeta, dx_split)."""
    R, C = _rc(x)
    assert _same_layout(dy, x)
    dx = torch.empty_like(x)
    dgamma = _out(out_dgamma, (C,), x.device) if need_affine_grads else None
    dbeta = _out(out_dbeta, (C,), x.device) if need_affine_grads else None
    ws = _ws(_lib.load().vp_bn_workspace_bytes(R, C), x)
    if want_split:
        dxs = empty_split(x.numel(), x)
        _lib.call("vp_bn_act_bwd_split_f32", _p(x), _p(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dx), _pv(dxs), _p(dgamma), _p(dbeta),
                  R, C, act, float(slope), int(batch_stats), _p(ws), ws.numel() * 4, _stream())
        return dx, dgamma, dbeta, dxs
    _lib.call("vp_bn_act_bwd_f32", _p(x), _p(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dx), _p(dgamma), _p(dbeta),
              R, C, act, float(slope), int(batch_stats), _p(ws), ws.numel() * 4, _stream())
    return dx, dgamma, dbeta


def instnorm_act_fwd(x, eps: float, act: int, slope: float = 0.0, want_split: bool = False):
    """x: (B, C, H, W) channels_last -> (y, mean[B][C], rstd[B][C]) (+ the bf16 hi/lo planes of y with ``want_split``, C % 4 == 0)."""
    B, C, H, W = x.shape
    y = torch.empty_like(x)
    mean = torch.empty((B, C), dtype=torch.float32, device=x.device)
    rstd = torch.empty((B, C), dtype=torch.float32, device=x.device)
    ws = _ws(_lib.load().vp_instnorm_workspace_bytes(B, H * W, C), x)
    if want_split:
        ys = empty_split(x.numel(), x)
        _lib.call("vp_instnorm_act_fwd_split_f32", _p(x), _p(y), _pv(ys), _p(mean), _p(rstd), B, H * W, C, eps, act, slope, _p(ws),
                  ws.numel() * 4, _stream())
        return y, mean, rstd, ys
    _lib.call("vp_instnorm_act_fwd_f32", _p(x), _p(y), _p(mean), _p(rstd), B, H * W, C, eps, act, slope, _p(ws), ws.numel() * 4, _stream())
    return y, mean, rstd


def instnorm_act_bwd(x, dy, mean, rstd, act: int, slope: float = 0.0, want_split: bool = False):
    B, C, H, W = x.shape
    dx = torch.empty_like(x)
    ws = _ws(_lib.load().vp_instnorm_workspace_bytes(B, H * W, C), x)
    if want_split:
        dxs = empty_split(x.numel(), x)
        _lib.call("vp_instnorm_act_bwd_split_f32", _p(x), _p(dy), _p(mean), _p(rstd), _p(dx), _pv(dxs), B, H * W, C, act, slope, _p(ws),
                  ws.numel() * 4, _stream())
        return dx, dxs
    _lib.call("vp_instnorm_act_bwd_f32", _p(x), _p(dy), _p(mean), _p(rstd), _p(dx), B, H * W, C, act, slope, _p(ws), ws.numel() * 4,
              _stream())
    return dx


def pair_blend_fwd(u, label, norm: bool, eps: float, act: int, slope: float = 0.0, want_split: bool = False):
    """u: (B, 2C, H, W) channels_last, the stacked convolution of a label-gated pair; label: (B,) float32 ->
    (y (B, C, H, W), mean[B][2C] | None, rstd[B][2C] | None, the bf16 hi/lo planes of y | None)."""
    B, C2, H, W = u.shape
    assert _is_nhwc(u) and C2 % 2 == 0 and label.shape == (B,)
    C = C2 // 2
    y = empty_cl(B, C, H, W, u)
    mean = rstd = ws = None
    if norm:
        mean = torch.empty((B, C2), dtype=torch.float32, device=u.device)
        rstd = torch.empty((B, C2), dtype=torch.float32, device=u.device)
        ws = _ws(_lib.load().vp_pair_blend_workspace_bytes(B, H * W, C), u)
    ys = empty_split(y.numel(), u) if want_split else None
    _lib.call("vp_pair_blend_fwd_f32", _p(u), _p(label), _p(y), _pv(ys), _p(mean), _p(rstd), B, H * W, C, int(norm), float(eps), act,
              float(slope), _p(ws), 0 if ws is None else ws.numel() * 4, _stream())
    return y, mean, rstd, ys


def pair_blend_bwd(u, dy, label, mean, rstd, norm: bool, act: int, slope: float = 0.0, want_split: bool = False):
    """Gradient of pair_blend_fwd with respect to u (the label is a constant): (du, the bf16 hi/lo planes of du | None)."""
    B, C2, H, W = u.shape
    C = C2 // 2
    assert _is_nhwc(u) and _is_nhwc(dy) and tuple(dy.shape) == (B, C, H, W)
    du = torch.empty_like(u)
    ws = _ws(_lib.load().vp_pair_blend_workspace_bytes(B, H * W, C), u) if norm else None
    dus = empty_split(u.numel(), u) if want_split else None
    _lib.call("vp_pair_blend_bwd_f32", _p(u), _p(dy), _p(label), _p(mean), _p(rstd), _p(du), _pv(dus), B, H * W, C, int(norm), act,
              float(slope), _p(ws), 0 if ws is None else ws.numel() * 4, _stream())
    return du, dus


def act_fwd(x, act: int, slope: float = 0.0):
    y = torch.empty_like(x)
    _lib.call("vp_act_fwd_f32", _p(x), _p(y), x.numel(), act, float(slope), _stream())
    return y


def act_bwd_from_y(y, dy, act: int, slope: float = 0.0):
    assert _same_layout(y, dy)
    dx = torch.empty_like(y)
    _lib.call("vp_act_bwd_from_y_f32", _p(y), _p(dy), _p(dx), y.numel(), act, float(slope), _stream())
    return dx


# ---- latent + loss ---------------------------------------------------------------------------------
def latent_fwd(mu, logvar, eps, want_kl: bool = True):
    B, Z = mu.shape
    mu, logvar, eps = mu.contiguous(), logvar.contiguous(), eps.contiguous()
    z = torch.empty_like(mu)
    kl = torch.empty((B,), dtype=torch.float32, device=mu.device) if want_kl else None
    _lib.call("vp_latent_fwd_f32", _p(mu), _p(logvar), _p(eps), _p(z), _p(kl), B, Z, _stream())
    return z, kl


def latent_bwd(mu, logvar, eps, dz, gkl, gkl_scalar: float = 0.0):
    B, Z = mu.shape
    dmu = torch.empty_like(mu)
    dlv = torch.empty_like(mu)
    _lib.call("vp_latent_bwd_f32", _p(mu.contiguous()), _p(logvar.contiguous()), _p(eps.contiguous()),
              _p(dz.contiguous() if dz is not None else None), _p(gkl.contiguous() if gkl is not None else None),
              float(gkl_scalar), _p(dmu), _p(dlv), B, Z, _stream())
    return dmu, dlv


def bce_sum(p, t):
    assert _same_layout(p, t)
    n = p.numel()
    ws = _ws(_lib.load().vp_reduce_workspace_bytes(n), p)
    out = torch.empty((1,), dtype=torch.float32, device=p.device)
    _lib.call("vp_bce_sum_f32", _p(p), _p(t), n, _p(out), _p(ws), ws.numel() * 4, _stream())
    return out


def bce_rows(p, t):
    """out[r] = the BCE sum over row r of p, t (rows, ...): the per-image reconstruction term"""
    assert _same_layout(p, t)
    if not (p.is_contiguous() or _is_nhwc(p)):      # rows must be the outermost, dense dimension (either image order will do)
        p, t = p.contiguous(), t.contiguous()
    rows, n = p.shape[0], p.numel() // p.shape[0]
    ws = _ws(_lib.load().vp_bce_rows_workspace_bytes(rows, n), p)
    out = torch.empty((rows,), dtype=torch.float32, device=p.device)
    _lib.call("vp_bce_rows_f32", _p(p), _p(t), rows, n, _p(out), _p(ws), ws.numel() * 4, _stream())
    return out


def latent_iw_fwd(mu, logvar, eps, want_kl: bool = True):
    """(z, kl, lr): latent_fwd's z and kl (the same bits) and lr[b] = log p(z_b) - log q(z_b | x_b)"""
    B, Z = mu.shape
    mu, logvar, eps = mu.contiguous(), logvar.contiguous(), eps.contiguous()
    z = torch.empty_like(mu)
    kl = torch.empty((B,), dtype=torch.float32, device=mu.device) if want_kl else None
    lr = torch.empty((B,), dtype=torch.float32, device=mu.device)
    _lib.call("vp_latent_iw_fwd_f32", _p(mu), _p(logvar), _p(eps), _p(z), _p(kl), _p(lr), B, Z, _stream())
    return z, kl, lr


def iw_bound(nbce, lr, want_logw: bool = True):
    """(logw, iwae) of nbce, lr (B, K): logw = lr - nbce, iwae[b] = log-mean-exp_k logw[b] (the K-sample importance-weighted bound)"""
    B, K = nbce.shape
    assert tuple(lr.shape) == (B, K)
    nbce, lr = nbce.contiguous(), lr.contiguous()
    logw = torch.empty_like(nbce) if want_logw else None
    iwae = torch.empty((B,), dtype=torch.float32, device=nbce.device)
    _lib.call("vp_iw_bound_f32", _p(nbce), _p(lr), B, K, _p(logw), _p(iwae), _stream())
    return logw, iwae


def bce_masked_rows_bwd(p, t, mask: Optional[torch.Tensor] = None):
    """(out, dlogit): out[r] = the mask-weighted BCE sum over row r of p, t (rows, ...), dlogit = mask * (p - t); mask None: all ones"""
    assert _same_layout(p, t) and (mask is None or _same_layout(p, mask))
    if not (p.is_contiguous() or _is_nhwc(p)):
        p, t, mask = p.contiguous(), t.contiguous(), None if mask is None else mask.contiguous()
    rows, n = p.shape[0], p.numel() // p.shape[0]
    ws = _ws(_lib.load().vp_bce_masked_rows_bwd_workspace_bytes(rows, n), p)
    out = torch.empty((rows,), dtype=torch.float32, device=p.device)
    dl = torch.empty_like(p)
    _lib.call("vp_bce_masked_rows_bwd_f32", _p(p), _p(t), _p(mask), rows, n, _p(out), _p(dl), _p(ws), ws.numel() * 4, _stream())
    return out, dl


def affine_relu_bwd(dy, u, scale, want_f32: bool = True, want_split: bool = False, inplace: bool = False):
    """(dx, dx_split) = backward through u = relu(scale * c + shift) from the output: dy * scale * (u > 0) over [R][C] with
    C = scale.numel().  ``u``: fp32, or (2, n) int16 split planes.  ``inplace``: dx is dy itself."""
    C = scale.numel()
    n = dy.numel()
    assert n % C == 0 and dy.is_contiguous() and u.is_contiguous() and (want_f32 or want_split)
    split_in = u.dtype == torch.int16
    assert u.numel() == (2 * n if split_in else n)
    dx = (dy if inplace else torch.empty_like(dy)) if want_f32 else None
    dxs = empty_split(n, dy) if want_split else None
    _lib.call("vp_affine_relu_bwd_f32", _p(dy), None if split_in else _p(u), _pv(u) if split_in else None, _p(scale), _p(dx),
              _pv(dxs), n // C, C, _stream())
    return dx, dxs


def bce_bwd(p, t, g: Optional[torch.Tensor], gscale: float = 1.0):
    assert _same_layout(p, t)
    dp = torch.empty_like(p)
    _lib.call("vp_bce_bwd_f32", _p(p), _p(t), _p(g), float(gscale), _p(dp), p.numel(), _stream())
    return dp


def bce_sigmoid_bwd(p, t, gscale: float):
    assert _same_layout(p, t)
    dl = torch.empty_like(p)
    _lib.call("vp_bce_sigmoid_bwd_f32", _p(p), _p(t), float(gscale), _p(dl), p.numel(), _stream())
    return dl


def global_avgpool_fwd(x):
    """x: (B, C, H, W) channels_last -> (B, C) means."""
    B, C, H, W = x.shape
    out = torch.empty((B, C), dtype=torch.float32, device=x.device)
    _lib.call("vp_global_avgpool_fwd_f32", _p(x), _p(out), B, H * W, C, _stream())
    return out


def global_avgpool_bwd(dy, shape):
    B, C, H, W = shape
    dx = empty_cl(B, C, H, W, dy)
    _lib.call("vp_global_avgpool_bwd_f32", _p(dy), _p(dx), B, H * W, C, _stream())
    return dx


def scse_workspace_bytes(B: int, HW: int, C: int, hidden: int) -> int:
    """Scratch bytes of scse_fwd / scse_bwd (0: the shape is refused); a host-side query, callable without a device."""
    return int(_lib.load().vp_scse_workspace_bytes(B, HW, C, hidden))


def _scse_hidden(x, w1) -> int:
    """C / reduction of the block, refused here when it is 0: before anything is allocated, in the C side's words."""
    Cr = w1.shape[0]
    if Cr == 0:
        raise _lib.VaePlayHipError(f"scse: hidden = 0 channels (C / reduction == 0 at C = {x.shape[1]}): the channel gate needs "
                                   "1 <= hidden <= C")
    return Cr


def scse_fwd(x, w1, b1, w2, b2, ws, bs, relu: bool = False):
    """SCSEBlock forward on a channels_last x: (y, pool (B, C), hid (B, C/r), cgate (B, C), sgate (B, H*W)); the last four are
    what scse_bwd needs besides x.  w1 (C/r, C, 1, 1), w2 (C, C/r, 1, 1), ws (1, C, 1, 1) are the reference's conv weights."""
    B, C, H, W = x.shape
    Cr = _scse_hidden(x, w1)
    assert _is_nhwc(x) and w1.shape[1] == C and tuple(w2.shape[:2]) == (C, Cr) and ws.numel() == C and bs.numel() == 1
    w1, b1, w2, b2, ws, bs = (t.contiguous() for t in (w1, b1, w2, b2, ws, bs))
    y = torch.empty_like(x)
    pool, cgate = (torch.empty((B, C), dtype=torch.float32, device=x.device) for _ in range(2))
    hid = torch.empty((B, Cr), dtype=torch.float32, device=x.device)
    sgate = torch.empty((B, H * W), dtype=torch.float32, device=x.device)
    wk = _ws(scse_workspace_bytes(B, H * W, C, Cr), x)
    _lib.call("vp_scse_fwd_f32", _p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(ws), _p(bs), _p(y), _p(pool), _p(hid), _p(cgate), _p(sgate),
              B, H * W, C, Cr, int(relu), _p(wk), wk.numel() * 4, _stream())
    return y, pool, hid, cgate, sgate


def scse_bwd(x, dy, w1, w2, ws, pool, hid, cgate, sgate, relu: bool = False, need_dx: bool = True, out=None):
    """Gradients of scse_fwd: (dx, dw1, db1, dw2, db2, dws, dbs), the parameter gradients in the shapes of the parameters.
    ``need_dx=False`` skips both passes that store dx (dx is then None); ``out`` may name, per parameter gradient, a contiguous
    tensor of the parameter's shape to write into (None entries get a fresh tensor)."""
    B, C, H, W = x.shape
    Cr = _scse_hidden(x, w1)
    assert _is_nhwc(x) and _same_layout(x, dy)
    w1, w2, ws = w1.contiguous(), w2.contiguous(), ws.contiguous()
    dx = torch.empty_like(x) if need_dx else None
    shapes = ((Cr, C, 1, 1), (Cr,), (C, Cr, 1, 1), (C,), (1, C, 1, 1), (1,))
    grads = []
    for shape, o in zip(shapes, out or (None,) * 6):
        if o is None:
            o = torch.empty(shape, dtype=torch.float32, device=x.device)
        assert tuple(o.shape) == shape and o.is_contiguous() and o.dtype == torch.float32
        grads.append(o)
    wk = _ws(scse_workspace_bytes(B, H * W, C, Cr), x)
    _lib.call("vp_scse_bwd_f32", _p(x), _p(dy), _p(w1), _p(w2), _p(ws), _p(pool), _p(hid), _p(cgate), _p(sgate),
              _p(dx) if need_dx else None, *(_p(g) for g in grads), B, H * W, C, Cr, int(relu), _p(wk), wk.numel() * 4, _stream())
    return (dx, *grads)


def twin_head_fwd(h_adv, h_aux, w_adv, b_adv, w_aux, b_aux):
    """The Style-GAN discriminator's output stage on the channels_last (B, C, 2, 2) outputs of adv_convs.0 / aux_convs.0:
    (adv (B, 1) = sigmoid, aux (B, K) = softmax) of the two 3x3 stride-2 convolutions, one launch.  w_adv (1, C, 3, 3),
    w_aux (K, C, 3, 3) are the reference's conv weights."""
    B, C, H, W = h_adv.shape
    K = w_aux.shape[0]
    assert (H, W) == (2, 2) and _is_nhwc(h_adv) and _is_nhwc(h_aux) and h_aux.shape == h_adv.shape
    assert tuple(w_adv.shape) == (1, C, 3, 3) and tuple(w_aux.shape) == (K, C, 3, 3) and b_adv.numel() == 1 and b_aux.numel() == K
    w_adv, b_adv, w_aux, b_aux = (t.contiguous() for t in (w_adv, b_adv, w_aux, b_aux))
    adv = torch.empty((B, 1), dtype=torch.float32, device=h_adv.device)
    aux = torch.empty((B, K), dtype=torch.float32, device=h_adv.device)
    _lib.call("vp_twin_head_fwd_f32", _p(h_adv), _p(h_aux), _p(w_adv), _p(b_adv), _p(w_aux), _p(b_aux), _p(adv), _p(aux), B, C, K, _stream())
    return adv, aux


def twin_head_bwd(h_adv, h_aux, w_adv, w_aux, adv, aux, d_adv, d_aux, out=None):
    """Gradients of twin_head_fwd: (dh_adv, dh_aux, dw_adv, db_adv, dw_aux, db_aux), one launch.  ``d_adv`` / ``d_aux`` may be None
    (that output did not reach the loss); ``out`` may name, per parameter gradient, a contiguous tensor of the parameter's shape to
    write into (None entries get a fresh tensor)."""
    B, C, H, W = h_adv.shape
    K = w_aux.shape[0]
    assert (H, W) == (2, 2) and _is_nhwc(h_adv) and _is_nhwc(h_aux) and h_aux.shape == h_adv.shape
    assert adv.is_contiguous() and aux.is_contiguous() and adv.numel() == B and tuple(aux.shape) == (B, K)
    w_adv, w_aux = w_adv.contiguous(), w_aux.contiguous()
    d_adv = None if d_adv is None else d_adv.contiguous()
    d_aux = None if d_aux is None else d_aux.contiguous()
    assert (d_adv is None or d_adv.numel() == B) and (d_aux is None or tuple(d_aux.shape) == (B, K))
    dh_adv, dh_aux = torch.empty_like(h_adv), torch.empty_like(h_aux)
    shapes = ((1, C, 3, 3), (1,), (K, C, 3, 3), (K,))
    grads = [_out(o, shape, h_adv.device) for shape, o in zip(shapes, out or (None,) * 4)]
    _lib.call("vp_twin_head_bwd_f32", _p(h_adv), _p(h_aux), _p(w_adv), _p(w_aux), _p(adv), _p(aux), _p(d_adv), _p(d_aux), _p(dh_adv),
              _p(dh_aux), *(_p(g) for g in grads), B, C, K, _stream())
    return (dh_adv, dh_aux, *grads)


def _attn_dims(q, k, v):
    B, N, dq = q.shape
    C = v.shape[2]
    assert tuple(k.shape) == (B, N, dq) and tuple(v.shape) == (B, N, C) and all(t.is_contiguous() for t in (q, k, v))
    return B, N, dq, C


def attention_bwd_workspace_bytes(B: int, N: int, dq: int, C: int) -> int:
    return int(_lib.load().vp_attn_bwd_workspace_bytes(B, N, dq, C))


def attention_fwd(q, k, v, x, gamma):
    """y = gamma * softmax(q k^T) v + x per image, one launch, no N x N map: contiguous q, k (B, N, dq), v, x (B, N, C), gamma (1,)
    on the device.  Returns (y, o, lse): o = softmax(q k^T) v (B, N, C) and lse (B, N) are what attention_bwd needs."""
    B, N, dq, C = _attn_dims(q, k, v)
    assert x.shape == v.shape and x.is_contiguous() and gamma.numel() == 1
    y, o = torch.empty_like(x), torch.empty_like(x)
    lse = torch.empty((B, N), dtype=torch.float32, device=x.device)
    _lib.call("vp_attn_fwd_f32", _p(q), _p(k), _p(v), _p(x), _p(gamma), _p(y), _p(o), _p(lse), B, N, dq, C, _stream())
    return y, o, lse


def attention_bwd(q, k, v, o, lse, g, gamma, need_q: bool = True, need_k: bool = True, need_v: bool = True):
    """Gradients of attention_fwd against the upstream gradient g (B, N, C): (dq, dk, dv, dgamma (1,)); a gradient that is not
    needed is None and its kernel is not launched.  The attention map is recomputed from lse; dx is g itself."""
    B, N, dq, C = _attn_dims(q, k, v)
    assert o.shape == v.shape and g.shape == v.shape and o.is_contiguous() and g.is_contiguous()
    assert tuple(lse.shape) == (B, N) and lse.is_contiguous() and gamma.numel() == 1
    d_q = torch.empty_like(q) if need_q else None
    d_k = torch.empty_like(k) if need_k else None
    d_v = torch.empty_like(v) if need_v else None
    dgamma = torch.empty(1, dtype=torch.float32, device=q.device)
    wk = _ws(attention_bwd_workspace_bytes(B, N, dq, C), q)
    _lib.call("vp_attn_bwd_f32", _p(q), _p(k), _p(v), _p(o), _p(lse), _p(g), _p(gamma), _p(d_q), _p(d_k), _p(d_v), _p(dgamma),
              _p(wk), wk.numel() * 4, B, N, dq, C, _stream())
    return d_q, d_k, d_v, dgamma


def softmax_rows_fwd(x2d):
    R, n = x2d.shape
    y = torch.empty_like(x2d)
    _lib.call("vp_softmax_rows_fwd_f32", _p(x2d), _p(y), R, n, _stream())
    return y


def cross_entropy_fwd(logits2d: torch.Tensor, labels: torch.Tensor):
    """F.cross_entropy (mean) of (R, n) logits against int64 labels: (loss (1,), softmax rows (R, n))."""
    R, n = logits2d.shape
    if labels.dtype != torch.int64 or labels.shape != (R,) or not labels.is_cuda:
        raise _lib.VaePlayHipError("cross_entropy: labels must be an int64 device tensor of shape (rows,)")
    loss = torch.empty(1, dtype=torch.float32, device=logits2d.device)
    prob = torch.empty_like(logits2d)
    _lib.call("vp_cross_entropy_fwd_f32", _p(logits2d), c_void_p(labels.data_ptr()), _p(loss), _p(prob), R, n, _stream())
    return loss, prob


def cross_entropy_bwd(prob: torch.Tensor, labels: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    R, n = prob.shape
    dx = torch.empty_like(prob)
    _lib.call("vp_cross_entropy_bwd_f32", _p(prob), c_void_p(labels.data_ptr()), _p(g), _p(dx), R, n, _stream())
    return dx


def softmax_rows_bwd(y2d, dy2d):
    R, n = y2d.shape
    dx = torch.empty_like(y2d)
    _lib.call("vp_softmax_rows_bwd_f32", _p(y2d), _p(dy2d), _p(dx), R, n, _stream())
    return dx


def l1_mean(a, b):
    n = a.numel()
    ws = _ws(2 * _lib.load().vp_reduce_workspace_bytes(n), a)
    out = torch.empty((1,), dtype=torch.float32, device=a.device)
    _lib.call("vp_l1_mean_f32", _p(a), _p(b), n, _p(out), _p(ws), ws.numel() * 4, _stream())
    return out


def l1_mean_bwd(a, b, g, want_a: bool, want_b: bool):
    da = torch.empty_like(a) if want_a else None
    db = torch.empty_like(a) if want_b else None
    _lib.call("vp_l1_mean_bwd_f32", _p(a), _p(b), _p(g), _p(da), _p(db), a.numel(), _stream())
    return da, db


def be_loss_fwd(logits, targets, bce_weight: float, smooth: float):
    B, n = logits.shape[0], logits.numel() // logits.shape[0]
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    sums = torch.empty((B, 4), dtype=torch.float32, device=logits.device)
    ws = _ws(_lib.load().vp_be_loss_workspace_bytes(B, n), logits)
    _lib.call("vp_be_loss_fwd_f32", _p(logits), _p(targets), _p(loss), _p(sums), B, n, bce_weight, smooth, _p(ws), ws.numel() * 4,
              _stream())
    return loss, sums


def be_loss_bwd(logits, targets, sums, g, bce_weight: float, smooth: float):
    B, n = logits.shape[0], logits.numel() // logits.shape[0]
    dx = torch.empty_like(logits)
    _lib.call("vp_be_loss_bwd_f32", _p(logits), _p(targets), _p(sums), _p(g), _p(dx), B, n, bce_weight, smooth, _stream())
    return dx


def dice_loss_fwd(probs, targets, smooth: float):
    B, n = probs.shape[0], probs.numel() // probs.shape[0]
    loss = torch.empty(1, dtype=torch.float32, device=probs.device)
    sums = torch.empty((B, 4), dtype=torch.float32, device=probs.device)
    ws = _ws(_lib.load().vp_be_loss_workspace_bytes(B, n), probs)
    _lib.call("vp_dice_loss_fwd_f32", _p(probs), _p(targets), _p(loss), _p(sums), B, n, smooth, _p(ws), ws.numel() * 4, _stream())
    return loss, sums


def dice_loss_bwd(probs, targets, sums, g, smooth: float):
    B, n = probs.shape[0], probs.numel() // probs.shape[0]
    dp = torch.empty_like(probs)
    _lib.call("vp_dice_loss_bwd_f32", _p(probs), _p(targets), _p(sums), _p(g), _p(dp), B, n, smooth, _stream())
    return dp


def half_sqdiff(a, b):
    out = torch.empty_like(a)
    _lib.call("vp_half_sqdiff_f32", _p(a), _p(b), _p(out), a.numel(), _stream())
    return out


def half_sqdiff_rowsum(a, b):
    R, n = a.shape[0], a.numel() // a.shape[0]
    out = torch.empty(R, dtype=torch.float32, device=a.device)
    _lib.call("vp_half_sqdiff_rowsum_f32", _p(a), _p(b), _p(out), R, n, _stream())
    return out


def half_sqdiff_bwd(a, b, g, per_row: bool, want_a: bool = True, want_b: bool = True):
    R, n = a.shape[0], a.numel() // a.shape[0]
    da = torch.empty_like(a) if want_a else None
    db = torch.empty_like(a) if want_b else None
    _lib.call("vp_half_sqdiff_bwd_f32", _p(a), _p(b), _p(g), _p(da), _p(db), R, n, 1 if per_row else 0, _stream())
    return da, db


def tensor_sum(x):
    n = x.numel()
    ws = _ws(_lib.load().vp_reduce_workspace_bytes(n), x)
    out = torch.empty((1,), dtype=torch.float32, device=x.device)
    _lib.call("vp_sum_f32", _p(x), n, _p(out), _p(ws), ws.numel() * 4, _stream())
    return out


# ---- optimiser -----------------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, beta1, beta2, eps, step: int, grad_scale: float = 1.0):
    _lib.call("vp_adam_f32", _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
              int(step), float(grad_scale), _stream())


def adam_outer_step(p2d, m2d, v2d, A, Bm, lr, beta1, beta2, eps, step: int, grad_scale: float = 1.0):
    """Adam on p2d [R][Cn] with the gradient grad_scale * A^T Bm (A [K][R], Bm [K][Cn]) contracted inside the update."""
    R, Cn = p2d.shape
    K = A.shape[0]
    assert A.shape == (K, R) and Bm.shape == (K, Cn) and A.is_contiguous() and Bm.is_contiguous() and p2d.is_contiguous()
    _lib.call("vp_adam_outer_f32", _p(p2d), _p(m2d), _p(v2d), _p(A), _p(Bm), K, R, Cn, lr, beta1, beta2, eps, step, grad_scale, _stream())


def rmsprop_step(p, g, sq, lr, alpha, eps, grad_scale: float = 1.0):
    _lib.call("vp_rmsprop_f32", _p(p), _p(g), _p(sq), p.numel(), float(lr), float(alpha), float(eps), float(grad_scale), _stream())


def latent_adam_step(z, g, m, v, step_count, lr, beta1, beta2, eps, prior_weight: float = 0.0, want_prior: bool = False):
    """One Adam step on latents z (rows, Z), in place, with gradient g + prior_weight * z; ``step_count``: int32 tensor of one
    element ON THE DEVICE holding the steps taken so far (read by the kernel, advanced by one behind it).  Returns
    prior[r] = prior_weight / 2 |z_r|^2 of the z it read, when asked."""
    rows, Z = z.shape
    assert z.is_contiguous() and all(t.is_contiguous() and t.shape == z.shape for t in (g, m, v))
    assert step_count.dtype == torch.int32 and step_count.is_cuda and step_count.numel() == 1
    prior = torch.empty((rows,), dtype=torch.float32, device=z.device) if want_prior else None
    _lib.call("vp_latent_adam_f32", _p(z), _p(g), _p(m), _p(v), _pv(step_count), rows, Z, float(lr), float(beta1), float(beta2),
              float(eps), float(prior_weight), _p(prior), _stream())
    return prior


def latent_prior(z, prior_weight: float):
    """prior[r] = prior_weight / 2 |z_r|^2, summed as latent_adam_step sums it (the same bits)"""
    rows, Z = z.shape
    assert z.is_contiguous()
    prior = torch.empty((rows,), dtype=torch.float32, device=z.device)
    _lib.call("vp_latent_adam_f32", _p(z), None, None, None, None, rows, Z, 0.0, 0.0, 0.0, 0.0, float(prior_weight), _p(prior), _stream())
    return prior


# ---- split-bf16 ("bf16x3") operands ----------------------------------------------------------------
# A split tensor is an int16 tensor of shape (2, n): plane 0 = bf16(x), plane 1 = bf16(x - plane0).
def _pv(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.VaePlayHipError("vae_play_amd ops need tensors on the HIP device (no CPU path exists)")
    return c_void_p(t.data_ptr())


def empty_split(n: int, like: torch.Tensor) -> torch.Tensor:
    return torch.empty((2, n), dtype=torch.int16, device=like.device)


PARAM_EPOCH = [0]        # bumped by every flat-arena optimiser step: the arena kernels change weights without touching torch's version counters

SPLIT_BF16, SPLIT_F16 = 0, 1     # VP_SPLIT_* of include/vaeplay_hip.h: bf16 pair ("bf16x3" kernels) | fp16 pair ("f16x2" kernels)


def split_f32(x: torch.Tensor, fmt: int = SPLIT_BF16, scale: float = 1.0) -> torch.Tensor:
    """Split planes of ``scale * x`` (scale: a power of two; gradients on the fp16-pair format, see the header)."""
    x = x if x.is_contiguous() or _is_nhwc(x) else x.contiguous()
    out = empty_split(x.numel(), x)
    if fmt == SPLIT_BF16 and scale == 1.0:
        _lib.call("vp_split_f32", _p(x), _pv(out), x.numel(), _stream())
    else:
        _lib.call("vp_split_fmt_f32", _p(x), _pv(out), x.numel(), fmt, scale, _stream())
    return out


def split_pad(x: torch.Tensor, cpad: int) -> torch.Tensor:
    """Split planes of an NHWC activation (logical (B, C, H, W), channels_last) with the channels zero-padded to ``cpad``."""
    B, C, H, W = x.shape
    x = x if _is_nhwc(x) else x.contiguous(memory_format=torch.channels_last)
    out = empty_split(B * H * W * cpad, x)
    _lib.call("vp_split_pad_f32", _p(x), _pv(out), B * H * W, C, cpad, _stream())
    return out


def unsplit(s: torch.Tensor, fmt: int = SPLIT_BF16) -> torch.Tensor:
    """hi + lo as fp32 (test helper; torch ops)."""
    dt = torch.float16 if fmt == SPLIT_F16 else torch.bfloat16
    return s[0].view(dt).float() + s[1].view(dt).float()


def pack_w5_split(w_ref: torch.Tensor, want_p0: bool, want_p1: bool, fmt: int = SPLIT_BF16):
    Cs, Cb = w_ref.shape[0], w_ref.shape[1]
    w_ref = w_ref.contiguous()
    n = Cs * Cb * 25
    p0 = empty_split(n, w_ref) if want_p0 else None
    p1 = empty_split(n, w_ref) if want_p1 else None
    if fmt == SPLIT_BF16:
        _lib.call("vp_pack_w5_split", _p(w_ref), _pv(p0), _pv(p1), Cs, Cb, _stream())
    else:
        job = (_lib.PackJob * 1)(_lib.PackJob(w_ref.data_ptr(), p0.data_ptr() if want_p0 else None, p1.data_ptr() if want_p1 else None,
                                               Cs, Cb, Cs, 2))
        _lib.call("vp_pack_w5_batch", job, 1, _stream())
    return p0, p1


def pack_w5_p1_split_padded(w_ref: torch.Tensor, cs_pad: int = 8) -> torch.Tensor:
    """Packed P1 split planes [Cbig][25][cs_pad] of a conv whose small side has 1 or 3 channels, zero-padded to ``cs_pad``
    (the narrow side of the final conv, models/networks.py:100-103): its input gradient then runs on the MFMA kernels."""
    Cs, Cb = w_ref.shape[0], w_ref.shape[1]
    w_ref = w_ref.contiguous()
    out = empty_split(Cb * 25 * cs_pad, w_ref)
    _lib.call("vp_pack_w5_p1_split_padded", _p(w_ref), _pv(out), Cs, Cb, cs_pad, _stream())
    return out


def conv5_gather_bf16x3(big_split, shape_big, w_p0_split, Cs: int, bias, stride: int, act: int = ACT_NONE):
    B, Cb, Hb, Wb = shape_big
    Hs, Ws = Hb // stride, Wb // stride
    out = torch.empty((B, Cs, Hs, Ws), dtype=torch.float32, device=big_split.device, memory_format=torch.channels_last)
    _lib.call("vp_conv5_gather_bf16x3", _pv(big_split), _pv(w_p0_split), _p(bias), _p(out), B, Hs, Ws, Cb, Cs, stride, act, _stream())
    return out


def conv5_scatter_bf16x3(small_split, shape_small, w_p1_split, Cb: int, stride: int):
    B, Cs, Hs, Ws = shape_small
    out = torch.empty((B, Cb, Hs * stride, Ws * stride), dtype=torch.float32, device=small_split.device,
                      memory_format=torch.channels_last)
    _lib.call("vp_conv5_scatter_bf16x3", _pv(small_split), _pv(w_p1_split), _p(out), B, Hs, Ws, Cs, Cb, stride, _stream())
    return out


def conv5_wgrad_bf16x3(big_split, shape_big, small_split, shape_small, stride: int, out: Optional[torch.Tensor] = None):
    B, Cb, Hb, Wb = shape_big
    _, Cs, Hs, Ws = shape_small
    nbytes = _lib.load().vp_conv5_wgrad_bf16x3_workspace_bytes(B, Hs, Ws, Cb, Cs, stride)
    ws = torch.empty(max(4, (nbytes + 3) // 4), dtype=torch.float32, device=big_split.device)
    dw = _out(out, (Cs, Cb, 5, 5), big_split.device)
    _lib.call("vp_conv5_wgrad_bf16x3", _pv(big_split), _pv(small_split), _p(dw), B, Hs, Ws, Cb, Cs, stride, _p(ws), ws.numel() * 4, _stream())
    return dw


# ---- 5x5 layers with a 1- or 3-channel side: the edge kernels (csrc/edge.hip) and the first conv as a 1x1 layer over its im2col ----
def conv5_smallin_fwd_bf16x3(x, weight, bias, act: int = ACT_NONE):
    """act(bias + conv5x5 stride 1) of a 1- | 3-channel fp32 NHWC image; weight (Cout, Cin, 5, 5) in the reference layout."""
    B, Cin, H, W = x.shape
    Cout = weight.shape[0]
    assert _is_nhwc(x) and weight.is_contiguous()
    y = empty_cl(B, Cout, H, W, x)
    _lib.call("vp_conv5_smallin_fwd_bf16x3", _p(x), _p(weight), _p(bias), _p(y), B, H, W, Cin, Cout, act, _stream())
    return y


def conv5_smallin_fwd_planes_bf16x3(x, weight, bias, act: int = ACT_NONE, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the same layer with the result written as split bf16 planes (2, B * H * W * Cout) int16 -- vp_split_f32 of the fp32 result, bit
    for bit -- into ``out`` when given"""
    B, Cin, H, W = x.shape
    Cout = weight.shape[0]
    assert _is_nhwc(x) and weight.is_contiguous()
    n = B * H * W * Cout
    out = empty_split(n, x) if out is None else out
    assert out.shape == (2, n) and out.dtype == torch.int16 and out.is_contiguous()
    _lib.call("vp_conv5_smallin_fwd_planes_bf16x3", _p(x), _p(weight), _p(bias), _pv(out), n, B, H, W, Cin, Cout, act, _stream())
    return out


def conv5_smallout_bf16x3(x, w_p0, bias, act: int = ACT_NONE):
    """act(bias + conv5x5 stride 1) down to 1 | 3 channels; x fp32 NHWC, w_p0 [Cout][25][Cin] fp32."""
    B, Cin, H, W = x.shape
    Cout = w_p0.shape[0]
    assert _is_nhwc(x) and w_p0.is_contiguous()
    y = empty_cl(B, Cout, H, W, x)
    _lib.call("vp_conv5_smallout_bf16x3", _p(x), _p(w_p0), _p(bias), _p(y), B, H, W, Cin, Cout, act, _stream())
    return y


def conv5_smallin_dgrad_bf16x3(dy, weight):
    """input gradient of a stride-1 5x5 conv whose OUTPUT has 1 | 3 channels; dy fp32 NHWC, weight (Cout, Cin, 5, 5)."""
    B, Cout, H, W = dy.shape
    Cin = weight.shape[1]
    assert _is_nhwc(dy) and weight.is_contiguous()
    dx = empty_cl(B, Cin, H, W, dy)
    _lib.call("vp_conv5_smallin_dgrad_bf16x3", _p(dy), _p(weight), _p(dx), B, H, W, Cout, Cin, _stream())
    return dx


def conv5_smallout_wgrad_bf16x3_workspace_bytes(B: int, H: int, W: int, Cin: int, Cout: int) -> int:
    """0: the kernel does not take this shape"""
    return _lib.load().vp_conv5_smallout_wgrad_bf16x3_workspace_bytes(B, H, W, Cin, Cout)


def conv5_smallout_wgrad_bf16x3(x, dy, out: Optional[torch.Tensor] = None):
    """dW (Cout, Cin, 5, 5) of a stride-1 5x5 conv down to 1 | 3 channels; x, dy fp32 NHWC."""
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    assert _is_nhwc(x) and _is_nhwc(dy)
    ws = _ws(conv5_smallout_wgrad_bf16x3_workspace_bytes(B, H, W, Cin, Cout), x)
    dw = _out(out, (Cout, Cin, 5, 5), x.device)
    _lib.call("vp_conv5_smallout_wgrad_bf16x3", _p(x), _p(dy), _p(dw), B, H, W, Cin, Cout, _p(ws), ws.numel() * 4, _stream())
    return dw


def im2col5s2_cols(C: int) -> int:
    """columns per output pixel of the 5x5 stride-2 im2col of a C-channel image (five kernel rows, padded)"""
    return _lib.load().vp_im2col5s2_cols(C)


def im2col5s2_split_f32(x, nchw: bool = False):
    """split planes [B * H/2 * W/2][im2col5s2_cols(C)] of the 5x5 stride-2 patches of an image (NHWC, or NCHW with ``nchw``)"""
    B, C, H, W = x.shape
    out = empty_split(B * (H // 2) * (W // 2) * im2col5s2_cols(C), x)
    _lib.call("vp_im2col5s2_split_f32", _p(x), _pv(out), B, C, H, W, int(nchw), _stream())
    return out


def pack_w_im2col5_split(weight):
    """weight (Cout, C, 5, 5) -> split planes [Cout][im2col5s2_cols(C)] in the im2col column order"""
    Cout, C = weight.shape[0], weight.shape[1]
    weight = weight.contiguous()
    out = empty_split(Cout * im2col5s2_cols(C), weight)
    _lib.call("vp_pack_w_im2col5_split", _p(weight), _pv(out), Cout, C, _stream())
    return out


def unpack_dw_im2col5_f32(dwc, C: int, out: Optional[torch.Tensor] = None):
    """dW in the im2col column order [Cout][im2col5s2_cols(C)] -> the reference layout (Cout, C, 5, 5)"""
    Cout = dwc.shape[0]
    dw = _out(out, (Cout, C, 5, 5), dwc.device)
    _lib.call("vp_unpack_dw_im2col5_f32", _p(dwc), _p(dw), Cout, C, _stream())
    return dw


# ---- fp16-pair operands: products = 3 (~1e-6 relative), 2 (two MFMAs per fragment pair, declared tolerance ~2e-4 per layer) or, gather
# and scatter only, 1 (hi planes only, one MFMA: inference, 11 significant bits per operand) ----
def conv5_gather_f16(big_split, shape_big, w_p0_split, Cs: int, bias, stride: int, act: int = ACT_NONE, products: int = 2,
                     out_scale: float = 1.0):
    B, Cb, Hb, Wb = shape_big
    Hs, Ws = Hb // stride, Wb // stride
    out = torch.empty((B, Cs, Hs, Ws), dtype=torch.float32, device=big_split.device, memory_format=torch.channels_last)
    _lib.call("vp_conv5_gather_f16", _pv(big_split), _pv(w_p0_split), _p(bias), _p(out), B, Hs, Ws, Cb, Cs, stride, act, products, out_scale,
              _stream())
    return out


def conv5_scatter_f16(small_split, shape_small, w_p1_split, Cb: int, stride: int, products: int = 2, out_scale: float = 1.0):
    B, Cs, Hs, Ws = shape_small
    out = torch.empty((B, Cb, Hs * stride, Ws * stride), dtype=torch.float32, device=small_split.device,
                      memory_format=torch.channels_last)
    _lib.call("vp_conv5_scatter_f16", _pv(small_split), _pv(w_p1_split), _p(out), B, Hs, Ws, Cs, Cb, stride, products, out_scale, _stream())
    return out


def conv5_wgrad_f16x2(big_split, shape_big, small_split, shape_small, stride: int, out_scale: float = 1.0):
    B, Cb, Hb, Wb = shape_big
    _, Cs, Hs, Ws = shape_small
    nbytes = _lib.load().vp_conv5_wgrad_bf16x3_workspace_bytes(B, Hs, Ws, Cb, Cs, stride)
    ws = torch.empty(max(4, (nbytes + 3) // 4), dtype=torch.float32, device=big_split.device)
    dw = torch.empty((Cs, Cb, 5, 5), dtype=torch.float32, device=big_split.device)
    _lib.call("vp_conv5_wgrad_f16x2", _pv(big_split), _pv(small_split), _p(dw), B, Hs, Ws, Cb, Cs, stride, out_scale, _p(ws),
              ws.numel() * 4, _stream())
    return dw


# ---- inference: eval-mode BatchNorm folded into the convolution's epilogue ---------------------
def bn_fold(gamma, beta, running_mean, running_var, eps: float):
    """(scale, shift, rstd) of an eval-mode BatchNorm: s = gamma / sqrt(var + eps), t = beta - mean s, rstd = 1 / sqrt(var + eps)"""
    C = running_mean.numel()
    scale, shift, rstd = (torch.empty(C, dtype=torch.float32, device=running_mean.device) for _ in range(3))
    _lib.call("vp_bn_fold_f32", _p(gamma), _p(beta), _p(running_mean), _p(running_var), float(eps), _p(scale), _p(shift), _p(rstd), C, _stream())
    return scale, shift, rstd


# ---- inference: the VAE-GAN discriminator's tap and head, the fold of two Linear layers (csrc/infer_gan.hip) ---------------------
def disc_tap_eval(c, scale, shift, act_flat=None, feat_flat=None, pair_rows: int = 0, dist=None) -> None:
    """c (n, 64, C) fp32 NHWC at 8x8 -> act_flat = relu(fma(c, scale, shift)) and feat_flat = c, (n, C * 64) in NCHW-flat order;
    dist[i] = 1/2 sum (c[i] - c[i + pair_rows])^2.  Outputs are written into the tensors given (None: not wanted)."""
    n, hw, C = c.shape
    assert hw == 64 and c.is_contiguous()
    _lib.call("vp_disc_tap_eval_f32", _p(c), _p(scale), _p(shift), n, C, _p(act_flat), _p(feat_flat), int(pair_rows), _p(dist), _stream())


def disc_head_eval(h, scale, shift, w, bias, logit=None, p=None, nl_real=None, nl_fake=None) -> None:
    """h (n, H): logit = sum relu(fma(h, scale, shift)) w + bias, p = sigmoid(logit), nl_real = -log(p + 1e-3),
    nl_fake = -log(1 - p + 1e-3), each (n,), written into the tensors given (None: not wanted)"""
    n, H = h.shape
    assert h.is_contiguous()
    _lib.call("vp_disc_head_eval_f32", _p(h), _p(scale), _p(shift), _p(w), _p(bias), n, H, _p(logit), _p(p), _p(nl_real), _p(nl_fake),
              _stream())


def lin_fold(w_out, b_out, w, b, w_new, b_new) -> None:
    """w_new (M, K) = w_out (M, N) w (N, K), b_new (M) = w_out b + b_out: two Linear layers without an activation between them as one"""
    M, N = w_out.shape
    K = w.shape[1]
    assert w.shape[0] == N and w_out.is_contiguous() and w.is_contiguous()
    _lib.call("vp_lin_fold_f32", _p(w_out), _p(b_out), _p(w), _p(b), M, N, K, _p(w_new), _p(b_new), _stream())


AFFINE_PRECISION = {"bf16x3": 0, "f32": 1, "f16": 2}      # precision codes of vp_conv5_affine_supported
OUT_BF16_PAIR, OUT_F16_PAIR, OUT_F16_HI = 0, 1, 2         # out_fmt of the vp_conv5_*_affine_f16 entry points


def conv5_affine_supported(family: int, precision: str, B: int, Hs: int, Ws: int, Cbig: int, Csmall: int, stride: int) -> bool:
    """does this launch shape take the affine epilogue?  family 0 = gather, 1 = scatter; precision "bf16x3" | "f32" | "f16" """
    return bool(_lib.load().vp_conv5_affine_supported(family, AFFINE_PRECISION[precision], B, Hs, Ws, Cbig, Csmall, stride))


def conv5_affine(family: int, precision: str, a, shape_a, w_packed, Cout: int, scale, shift, stride: int, act: int = ACT_RELU,
                 want_f32: bool = True, want_split: bool = False, out_fmt: int = OUT_BF16_PAIR, out_split=None):
    """act(scale * conv(a) + shift) in one launch.  ``a``: the input of logical shape ``shape_a`` (B, Cin, H, W) -- split planes
    (bf16x3: bf16 pairs; f16: fp16 planes, of which the one-product contraction reads the hi plane only) or a channels_last fp32
    tensor (f32); ``w_packed``: P0 (gather) / P1 (scatter) in the same arithmetic.  Returns (fp32 output or None, split planes or
    None); the f32 entry points refuse ``want_split``.  "f16" only: ``out_fmt`` = what the split planes hold (OUT_BF16_PAIR |
    OUT_F16_PAIR | OUT_F16_HI: the hi plane only, the lo plane of the buffer is left as it was); ``out_split``: write into this
    buffer instead of a new one."""
    B, Cin, H, W = shape_a
    Hs, Ws = (H // stride, W // stride) if family == 0 else (H, W)
    Ho, Wo = (Hs, Ws) if family == 0 else (H * stride, W * stride)
    out = torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device=a.device, memory_format=torch.channels_last) if want_f32 else None
    out_s = (out_split if out_split is not None else empty_split(B * Cout * Ho * Wo, a)) if want_split else None
    name = ("vp_conv5_gather_affine_", "vp_conv5_scatter_affine_")[family] + precision
    pa, pw = (_pv(a), _pv(w_packed)) if precision != "f32" else (_p(a), _p(w_packed))
    tail = (out_fmt,) if precision == "f16" else ()
    _lib.call(name, pa, pw, _p(scale), _p(shift), _p(out), _pv(out_s), B, Hs, Ws, Cin, Cout, stride, act, *tail, _stream())
    return out, out_s


# ---- k x k convolution families (models/blocks.py vocabulary) ------------------------------------------------
def pack_w(w_ref: torch.Tensor, want_p0: bool, want_p1: bool):
    """w_ref [Cs][Cb][k][k] -> p0 [Cs][k*k][Cb], p1 [Cb][k*k][Cs]."""
    Cs, Cb, ks = w_ref.shape[0], w_ref.shape[1], w_ref.shape[2]
    assert w_ref.shape[3] == ks
    w_ref = w_ref.contiguous()
    p0 = torch.empty((Cs, ks * ks, Cb), dtype=torch.float32, device=w_ref.device) if want_p0 else None
    p1 = torch.empty((Cb, ks * ks, Cs), dtype=torch.float32, device=w_ref.device) if want_p1 else None
    _lib.call("vp_pack_w_f32", _p(w_ref), _p(p0), _p(p1), Cs, Cb, ks, _stream())
    return p0, p1


def conv_out_size(n: int, ks: int, stride: int) -> int:
    return (n + 2 * ((ks - 1) // 2) - ks) // stride + 1


def conv_gather(big, w_p0, bias, ks: int, stride: int, act: int = ACT_NONE):
    assert _is_nhwc(big)
    B, Cb, Hb, Wb = big.shape
    Cs = w_p0.shape[0]
    Hs, Ws = conv_out_size(Hb, ks, stride), conv_out_size(Wb, ks, stride)
    out = empty_cl(B, Cs, Hs, Ws, big)
    _lib.call("vp_conv_gather_f32", _p(big), _p(w_p0), _p(bias), _p(out), B, Hs, Ws, Hb, Wb, Cb, Cs, ks, stride, act, _stream())
    return out


def conv_scatter(small, w_p1, ks: int, stride: int, Hb: int, Wb: int):
    assert _is_nhwc(small)
    B, Cs, Hs, Ws = small.shape
    Cb = w_p1.shape[0]
    out = empty_cl(B, Cb, Hb, Wb, small)
    _lib.call("vp_conv_scatter_f32", _p(small), _p(w_p1), _p(out), B, Hs, Ws, Hb, Wb, Cs, Cb, ks, stride, _stream())
    return out


def conv_scatter_bias(small, w_p1, bias: Optional[torch.Tensor], ks: int, stride: int, Hb: int, Wb: int):
    """conv_scatter + bias[Cb] on every output pixel in the same launch (nn.ConvTranspose2d's forward, models/network_Style_GAN.py:49,116)."""
    assert _is_nhwc(small)
    B, Cs, Hs, Ws = small.shape
    Cb = w_p1.shape[0]
    assert bias is None or (bias.shape == (Cb,) and bias.is_contiguous())
    out = empty_cl(B, Cb, Hb, Wb, small)
    _lib.call("vp_conv_scatter_bias_f32", _p(small), _p(w_p1), _p(bias), _p(out), B, Hs, Ws, Hb, Wb, Cs, Cb, ks, stride, _stream())
    return out


def conv_wgrad(big, small, ks: int, stride: int, out: Optional[torch.Tensor] = None):
    assert _is_nhwc(big) and _is_nhwc(small)
    B, Cb, Hb, Wb = big.shape
    _, Cs, Hs, Ws = small.shape
    nbytes = _lib.load().vp_conv_wgrad_workspace_bytes(B, Hs, Ws, Hb, Wb, Cb, Cs, ks, stride)
    ws = _ws(nbytes, big)
    dw = _out(out, (Cs, Cb, ks, ks), big.device)
    _lib.call("vp_conv_wgrad_f32", _p(big), _p(small), _p(dw), B, Hs, Ws, Hb, Wb, Cb, Cs, ks, stride, _p(ws), ws.numel() * 4, _stream())
    return dw


# ---- k x k split-bf16 ("bf16x3") forms ---------------------------------------------------------------------------------
def pack_w_split(w_ref: torch.Tensor, want_p0: bool, want_p1: bool):
    Cs, Cb, ks = w_ref.shape[0], w_ref.shape[1], w_ref.shape[2]
    w_ref = w_ref.contiguous()
    n = Cs * Cb * ks * ks
    p0 = empty_split(n, w_ref) if want_p0 else None
    p1 = empty_split(n, w_ref) if want_p1 else None
    _lib.call("vp_pack_w_split", _p(w_ref), _pv(p0), _pv(p1), Cs, Cb, ks, _stream())
    return p0, p1


def conv_gather_bf16x3(big_split, shape_big, w_p0_split, Cs: int, bias, ks: int, stride: int, act: int = ACT_NONE):
    B, Cb, Hb, Wb = shape_big
    Hs, Ws = conv_out_size(Hb, ks, stride), conv_out_size(Wb, ks, stride)
    out = torch.empty((B, Cs, Hs, Ws), dtype=torch.float32, device=big_split.device, memory_format=torch.channels_last)
    _lib.call("vp_conv_gather_bf16x3", _pv(big_split), _pv(w_p0_split), _p(bias), _p(out), B, Hs, Ws, Hb, Wb, Cb, Cs, ks, stride, act,
              _stream())
    return out


def conv_scatter_bf16x3(small_split, shape_small, w_p1_split, Cb: int, ks: int, stride: int, Hb: int, Wb: int):
    B, Cs, Hs, Ws = shape_small
    out = torch.empty((B, Cb, Hb, Wb), dtype=torch.float32, device=small_split.device, memory_format=torch.channels_last)
    _lib.call("vp_conv_scatter_bf16x3", _pv(small_split), _pv(w_p1_split), _p(out), B, Hs, Ws, Hb, Wb, Cs, Cb, ks, stride, _stream())
    return out


def conv_scatter_bias_bf16x3(small_split, shape_small, w_p1_split, bias: Optional[torch.Tensor], Cb: int, ks: int, stride: int, Hb: int,
                             Wb: int):
    B, Cs, Hs, Ws = shape_small
    assert bias is None or (bias.shape == (Cb,) and bias.is_contiguous())
    out = torch.empty((B, Cb, Hb, Wb), dtype=torch.float32, device=small_split.device, memory_format=torch.channels_last)
    _lib.call("vp_conv_scatter_bias_bf16x3", _pv(small_split), _pv(w_p1_split), _p(bias), _p(out), B, Hs, Ws, Hb, Wb, Cs, Cb, ks, stride,
              _stream())
    return out


def conv_wgrad_bf16x3(big_split, shape_big, small_split, shape_small, ks: int, stride: int, out: Optional[torch.Tensor] = None):
    B, Cb, Hb, Wb = shape_big
    _, Cs, Hs, Ws = shape_small
    nbytes = _lib.load().vp_conv_wgrad_bf16x3_workspace_bytes(B, Hs, Ws, Hb, Wb, Cb, Cs, ks, stride)
    ws = _ws(nbytes, big_split)
    dw = _out(out, (Cs, Cb, ks, ks), big_split.device)
    _lib.call("vp_conv_wgrad_bf16x3", _pv(big_split), _pv(small_split), _p(dw), B, Hs, Ws, Hb, Wb, Cb, Cs, ks, stride, _p(ws),
              ws.numel() * 4, _stream())
    return dw


def upsample2x_fwd(x):
    assert _is_nhwc(x)
    B, C, H, W = x.shape
    y = empty_cl(B, C, 2 * H, 2 * W, x)
    _lib.call("vp_upsample2x_bilinear_fwd_f32", _p(x), _p(y), B, H, W, C, _stream())
    return y


def upsample2x_bwd(dy):
    assert _is_nhwc(dy)
    B, C, Ho, Wo = dy.shape
    dx = empty_cl(B, C, Ho // 2, Wo // 2, dy)
    _lib.call("vp_upsample2x_bilinear_bwd_f32", _p(dy), _p(dx), B, Ho // 2, Wo // 2, C, _stream())
    return dx


def add_coords(x, normalize: bool):
    assert _is_nhwc(x)
    B, C, H, W = x.shape
    out = empty_cl(B, C + 2, H, W, x)
    _lib.call("vp_add_coords_f32", _p(x), _p(out), B, H, W, C, int(normalize), _stream())
    return out


def slice_channels(x, Cout: int):
    assert _is_nhwc(x)
    B, C, H, W = x.shape
    out = empty_cl(B, Cout, H, W, x)
    _lib.call("vp_slice_channels_f32", _p(x), _p(out), B * H * W, C, Cout, _stream())
    return out
