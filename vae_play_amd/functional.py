"""Autograd glue: each op of the VAE step as a torch.autograd.Function whose forward and
backward are HIP kernels (via ops.py -> C ABI).  This is what lets the reference's
``loss.backward()`` idiom (train_BE.py:63) work unchanged on the drop-in modules.

Reference ops replaced (relative to the reference checkout):
  conv5x5            nn.Conv2d(k5,p2,stride)                    models/networks.py:14,100          (_Conv, family "conv5x5")
  conv2d             nn.Conv2d(k in 1|3|4|5, p (k-1)//2, stride)  models/blocks.py:9-17            (_Conv, family "conv2d")
  conv_transpose5x5  nn.ConvTranspose2d(k5,s2,p2,op1)           models/networks.py:38              (_ConvT)
  batch_norm_act     nn.BatchNorm2d/1d + F.relu (+ blocks acts) models/networks.py:16,28-29,66-67; models/blocks.py:19-30
  conv_transpose2d   nn.ConvTranspose2d(k4,s2,p1) + bias          models/network_Style_GAN.py:49,116 (_ConvT)
  pair_blend         myConv2d: norm + act + label blend of a stacked conv   models/network_Style_GAN.py:72-79
  twin_head          Discriminator's two output convs + sigmoid / softmax   models/network_Style_GAN.py:214-229
  linear             nn.Linear                                  models/networks.py:65,69-70,88
  reparameterize     VaeGan.reparameterize                      models/networks.py:228-231
  kl_divergence      VaeGan.loss (kl term)                      models/networks.py:270
  binary_cross_entropy  F.binary_cross_entropy                  train_BE_font.py:107
  self_attention     SelfAttentionBlock's bmm / softmax / bmm   models/blocks.py:84-95             (_SelfAttentionFused | _SelfAttention)
"""
from __future__ import annotations

import collections
import os
import weakref

from typing import Optional

import torch
from torch.autograd import Function

from . import ops
from .ops import ACT_CODES, ACT_NONE, ACT_SIGMOID


def _cl(t: torch.Tensor) -> torch.Tensor:
    return ops.channels_last(t)


_PRECISION = "f32"


def set_conv_precision(mode: str) -> None:
    """Arithmetic of the 5x5 convolutions on the autograd front end: "f32" (exact fp32 MFMA, default) or "bf16x3"
    (split-bf16: three bf16 MFMAs per product, ~5e-6 relative error, ~3x the matrix rate; used where both channel
    counts are multiples of 8).  The fused engine has its own ``precision=`` argument."""
    global _PRECISION
    if mode not in ("f32", "bf16x3"):
        raise ValueError("precision must be 'f32' or 'bf16x3'")
    _PRECISION = mode


def get_conv_precision() -> str:
    return _PRECISION


_SMALL3 = True               # VALU kernels for the few-channel 3x3 convolutions (5.8 -> 3.8 ms per BE-heads step, profiles/r02_notes.md section 8)
_SMALL3_ALL = True
_BWD_SPLIT = True            # BatchNorm backward emits the split planes of dx


def _split_of(x: torch.Tensor) -> torch.Tensor:
    """bf16 hi/lo planes of an NHWC activation: the copy its producer emitted in the same pass (a BatchNorm+activation
    output in bf16x3 mode carries one, valid while the tensor has not been written since), else a split pass."""
    c = getattr(x, "_vp_split", None)
    if c is not None and c[1] == x._version and c[0].numel() == 2 * x.numel():
        return c[0]
    return ops.split_f32(x)


def _grad_out(param) -> Optional[torch.Tensor]:
    """Where a backward pass may WRITE ``param``'s gradient instead of returning a fresh tensor: its slice of the optimiser's flat
    gradient arena, when the parameter lives in one (optim.FlatArena) and has no gradient yet (``module.zero_grad()`` of
    train.py:68, or ``optimizer.zero_grad(set_to_none=True)``).  autograd's AccumulateGrad then adopts that view as ``.grad``
    without a kernel, where it would otherwise add a fresh tensor onto the zeroed arena -- one small add per parameter tensor
    and step (114 launches, 6 % of the VAE-GAN step).  A parameter used twice in one graph gets the view once (its hook clears
    the marker after accumulation); further contributions take the ordinary path and are added by autograd."""
    if param is None or not param.is_leaf or param.grad is not None or not _DIRECT_GRADS:      # (not a leaf: myConv2d's stacked weight)
        return None
    arena = getattr(param, "_vp_arena", None)
    if arena is None or getattr(param, "_vp_pending", False) or torch.is_grad_enabled():
        return None
    param._vp_pending = True
    return arena.grad_view(param)


_DIRECT_GRADS = True         # parameter gradients written straight into the arena slices (8.20 -> 8.00 ms per VAE-GAN step)


_PACKED = {}     # (id(weight), layout) -> (weakref(weight), weight._version, optimiser epoch, data_ptr, device, packed tensor)


def _evict_packed(wid: int) -> None:
    for k in [k for k in _PACKED if k[0] == wid]:
        _PACKED.pop(k, None)


def _packed(fn, weight, want_p1: bool):
    """``fn(weight, want_p0, want_p1)`` (an ops.pack_* re-layout of a conv weight) through a cache: a layer that runs several times
    per step -- the VAE-GAN's decoder decodes z and z_p, its discriminator sees both -- packs each layout once per weight VALUE.
    Valid while neither torch (``_version``) nor a flat-arena optimiser (ops.PARAM_EPOCH: its kernels update the weights behind
    torch's back) has changed the parameter and its storage is where it was (``module.to()`` / ``.float()`` re-point ``.data``
    without bumping the version); only leaf parameters are cached, and an entry dies with its parameter (weakref.finalize).
    Writes through ``p.data`` that keep the storage (``p.data.mul_()``, ``dist.broadcast(p.data)``) bump neither counter: follow them
    with ``ops.PARAM_EPOCH[0] += 1``."""
    if not (isinstance(weight, torch.nn.Parameter) and _PACK_CACHE_ON):
        r = fn(weight, not want_p1, want_p1)
        return r[1] if want_p1 else r[0]
    key = (id(weight), fn.__name__, want_p1, _PRECISION)
    hit = _PACKED.get(key)
    if (hit is not None and hit[0]() is weight and hit[1] == weight._version and hit[2] == ops.PARAM_EPOCH[0]
            and hit[3] == weight.data_ptr() and hit[4] == weight.device):
        return hit[5]
    r = fn(weight, not want_p1, want_p1)
    t = r[1] if want_p1 else r[0]
    if not any(k[0] == id(weight) for k in _PACKED):      # first entry of this parameter: drop its entries when it dies
        weakref.finalize(weight, _evict_packed, id(weight))
    _PACKED[key] = (weakref.ref(weight), weight._version, ops.PARAM_EPOCH[0], weight.data_ptr(), weight.device, t)
    return t


_PACK_CACHE_ON = True


def _smallin_shape(precision: str, Cout: int, Cin: int, stride: int) -> bool:
    return precision == "bf16x3" and stride == 1 and Cin in (1, 3) and Cout in (32, 64)


def first_conv_s1_edge(weight, stride: int) -> bool:
    """Does conv5x5(x, weight, bias, stride) run on the rows-in-K forward kernel (which takes a ReLU in its epilogue)?"""
    return _smallin_shape(_PRECISION, weight.shape[0], weight.shape[1], stride)


# ---- convolutions: route choice (pure functions of the geometry), one dense core, two Functions ---------------------------------
_Route = collections.namedtuple("_Route", "fwd dx dw")       # the kernels of the forward pass, the input and the weight gradient


def _conv_route(precision: str, small3: bool, small3_all: bool, family: str, Cout: int, Cin: int, ks: int, stride: int, act: int,
                has_bias: bool, B: int, H: int, W: int) -> _Route:
    """Which kernels run a convolution of the ``family`` "conv5x5" | "conv2d" (precision: get_conv_precision(); small3, small3_all:
    the module flags; B, H, W: the input).  Names: "f32" / "x16" the dense core on exact-fp32 / split-bf16 operands (x16: both
    channel counts multiples of 8), "padded" the split-bf16 core with the channel counts zero-padded to multiples of 8, "small3"
    the few-channel VALU kernels, the others the 5x5 special cases for a 1- | 3-channel side.

    The two families keep their own lists: conv2d never takes the 5x5 edge routes and conv5x5 never small3 / padded, as before
    they shared a front end.  One list would move some shapes to other kernels (conv2d with ks = 5 on a 64 -> 1 layer would go to
    the edge kernels): a performance change that needs measurements of its own."""
    bf = precision == "bf16x3"
    x16 = bf and Cout % 8 == 0 and Cin % 8 == 0
    if family == "conv2d":
        s3 = small3 and ks == 3 and stride == 1 and ops.conv3_small_wgrad_applicable(B, H, W, Cin, Cout)
        if s3 and small3_all:
            return _Route("small3", "small3", "small3")
        base = "x16" if x16 else ("padded" if bf else "f32")
        return _Route(base, base, "small3" if s3 else base)
    if bf and stride == 2 and Cin in (1, 3) and Cout % 8 == 0 and act == ACT_NONE and not has_bias and H % 2 == 0 and W % 2 == 0:
        return _Route("im2col", "scatter_padded", "im2col")
    if _smallin_shape(precision, Cout, Cin, stride) and act in (ACT_NONE, ops.ACT_RELU):
        return _Route("smallin", "smallout_flipped", "f32")
    if x16 and act in (ACT_NONE, ACT_SIGMOID):
        return _Route("x16", "x16", "x16")
    smallout = bf and stride == 1 and Cin == 64 and Cout in (1, 3) and act in (ACT_NONE, ACT_SIGMOID)
    if smallout:
        dx = "smallin_dgrad"
    elif bf and Cout < 8 and Cin % 8 == 0 and stride == 1:
        dx = "halo_padded"
    elif bf and Cin in (1, 3) and Cout in (32, 64) and stride == 1:
        dx = "smallout_flipped"
    elif bf and Cin < 8 and Cout % 8 == 0:
        dx = "scatter_padded"
    else:
        dx = "f32"
    dw = "smallout_wgrad" if smallout and ops.conv5_smallout_wgrad_bf16x3_workspace_bytes(B, H, W, Cin, Cout) else "f32"
    return _Route("smallout" if smallout else "f32", dx, dw)


def _convt_route(precision: str, Cin: int, Cout: int) -> str:
    """Which dense core runs a transposed convolution: "x16" (split-bf16) | "f32"."""
    return "x16" if precision == "bf16x3" and Cin % 8 == 0 and Cout % 8 == 0 else "f32"


# The dense core: gather, scatter and weight gradient of a ks x ks, stride s layer with weight (Csmall, Cbig, ks, ks).  An operand is
# the split planes of an activation (int16; the split-bf16 kernels) or the fp32 NHWC activation itself (the exact-fp32 kernels).
def _is_split(t: torch.Tensor) -> bool:
    return t.dtype == torch.int16


def _gather(big, shape_big, weight, bias, stride: int, act: int = ACT_NONE):
    """small = act(bias + conv(big))"""
    ks = weight.shape[2]
    if _is_split(big):
        return ops.conv_gather_bf16x3(big, shape_big, _packed(ops.pack_w_split, weight, False), weight.shape[0], bias, ks, stride, act)
    return ops.conv_gather(big, _packed(ops.pack_w, weight, False), bias, ks, stride, act)


def _scatter(small, shape_small, weight, bias, stride: int, Hb: int, Wb: int):
    """big (Hb x Wb) = bias + convT(small): a transposed convolution's forward pass, a convolution's input gradient"""
    ks = weight.shape[2]
    if _is_split(small):
        return ops.conv_scatter_bias_bf16x3(small, shape_small, _packed(ops.pack_w_split, weight, True), bias, weight.shape[1], ks, stride,
                                            Hb, Wb)
    return ops.conv_scatter_bias(small, _packed(ops.pack_w, weight, True), bias, ks, stride, Hb, Wb)


def _wgrad(big, shape_big, small, shape_small, ks: int, stride: int, param=None):
    """dW (Csmall, Cbig, ks, ks), written into ``param``'s arena slice where _grad_out offers one"""
    out = _grad_out(param)
    if _is_split(big):
        return ops.conv_wgrad_bf16x3(big, shape_big, small, shape_small, ks, stride, out=out)
    return ops.conv_wgrad(big, small, ks, stride, out=out)


def _bias_grad(dy, bias):
    B, C, H, W = dy.shape
    return ops.colsum(dy.permute(0, 2, 3, 1).reshape(B * H * W, C), out=_grad_out(bias))


def _pad8(c: int) -> int:
    return (c + 7) // 8 * 8


def _pad_w(weight, Cop: int, Cip: int):
    Co, Ci = weight.shape[0], weight.shape[1]
    return torch.nn.functional.pad(weight, (0, 0, 0, 0, 0, Cip - Ci, 0, Cop - Co)) if (Cop != Co or Cip != Ci) else weight


class _Conv(Function):
    """small = act(bias + conv(big)): kernel k in {1,3,4,5}, stride 1|2, padding (k-1)//2; weight (Csmall, Cbig, k, k) = nn.Conv2d
    layout.  ``family``: "conv5x5" (the VAE's layers, models/networks.py:14,100) | "conv2d" (models/blocks.py:9-17), see _conv_route."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride: int, act: int, family: str):
        x = _cl(x)
        B, Ci, H, W = x.shape
        Co = weight.shape[0]
        r = _conv_route(_PRECISION, _SMALL3, _SMALL3_ALL, family, Co, Ci, weight.shape[2], stride, act, bias is not None, B, H, W)
        a = x               # the operand the weight gradient reads
        if r.fwd == "im2col":
            # first conv on a 1- / 3-channel image (models/networks.py:14 via :55): its im2col written once as split planes, then a
            # 1x1 layer on the split-bf16 kernels for the forward pass and the weight gradient (as the fused step does)
            a = ops.im2col5s2_split_f32(x)
            y = ops.conv_gather_bf16x3(a, (B, ops.im2col5s2_cols(Ci), H // 2, W // 2), ops.pack_w_im2col5_split(weight), Co, None, 1, 1)
        elif r.fwd == "smallin":
            # stride-1 first conv on a 1- / 3-channel image (the VAE-GAN discriminator's, models/networks.py:160-163) with bias and
            # ReLU in the epilogue: a kernel row of taps per MFMA k-step (csrc/edge.hip, the rows-in-K kernel's forward form)
            y = ops.conv5_smallin_fwd_bf16x3(x, weight.contiguous(), bias, act)
        elif r.fwd == "small3":
            # a handful of channels on both sides (the networks_BE heads): one output pixel per thread, no packing / padding / split
            # -- exact-fp32 VALU kernels (csrc/small3.hip) instead of a 64 x 64 MFMA tile that is 92 - 98 % padding
            y = ops.conv3_small_fwd(x, weight.contiguous(), bias)
        elif r.fwd == "padded":
            # a channel count that is not a multiple of 8 on either side (32 + 2 coordinate channels in, 1 or 2 channels out):
            # zero-pad it to the next multiple of 8 and stay on the split-bf16 kernels -- the exact-f32 tile kernels run these
            # shapes with 70-97 % padding of their own (networks_BE heads: 65 % of the step in one f32 weight-gradient kernel)
            Cop, Cip = _pad8(Co), _pad8(Ci)
            bp = bias if (bias is None or Cop == Co) else torch.nn.functional.pad(bias, (0, Cop - Co))
            a = ops.split_pad(x, Cip) if Cip != Ci else _split_of(x)
            y = _gather(a, (B, Cip, H, W), _pad_w(weight, Cop, Cip), bp, stride)
            y = y[:, :Co] if Cop != Co else y
        elif r.fwd == "smallout":
            # the image side of the final conv (64 -> 1 | 3 channels, models/networks.py:100-103) on the matrix cores: the edge
            # kernels of the fused step (taps in the MFMA columns / rows, a kernel row per k-step) instead of the VALU kernels
            y = ops.conv5_smallout_bf16x3(x, _packed(ops.pack_w, weight, False), bias, act)
        else:                   # "x16" | "f32"
            a = _split_of(x) if r.fwd == "x16" else x
            y = _gather(a, x.shape, weight, bias, stride, act)
        ctx.route, ctx.stride, ctx.act, ctx.xshape = r, stride, act, tuple(x.shape)
        ctx.bias_param = bias
        ctx.save_for_backward(a, weight, y if act != ACT_NONE else None, x if r.dw == "small3" else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, weight, y, x32 = ctx.saved_tensors
        r, stride = ctx.route, ctx.stride
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        dy = _cl(dy)
        if ctx.act != ACT_NONE:
            dy = ops.act_bwd_from_y(y, dy, ctx.act)
        B, Ci, H, W = ctx.xshape
        Co, ks = weight.shape[0], weight.shape[2]
        Cop, Cip = (_pad8(Co), _pad8(Ci)) if r.fwd == "padded" else (Co, Ci)
        sshape = (B, Cop, dy.shape[2], dy.shape[3])
        dx = dw = db = None
        if need_dw and r.dw == "small3":
            dw = ops.conv3_small_wgrad(x32, dy, out=_grad_out(weight))
        if r.fwd == "padded":
            dys = ops.split_pad(dy, Cop) if Cop != Co else _split_of(dy)
        else:
            dys = _split_of(dy) if (r.fwd == "x16" or (need_dw and r.dw == "im2col")) else None
        if need_dw and r.dw == "im2col":
            dwc = _wgrad(a, (B, ops.im2col5s2_cols(Ci), H // 2, W // 2), dys, sshape, 1, 1)      # [Co][KC] in column order
            dw = ops.unpack_dw_im2col5_f32(dwc, Ci, out=_grad_out(weight))
        if need_dx:
            if r.dx == "small3":
                dx = ops.conv3_small_dgrad(dy, weight.contiguous())
            elif r.dx == "smallin_dgrad":
                dx = ops.conv5_smallin_dgrad_bf16x3(dy, weight.contiguous())
            elif r.dx == "halo_padded":
                # the image side of the final conv (1 or 3 channels): pad it to 8 channels and run the input gradient on
                # the split-bf16 halo kernel like the fused engine does (the exact-f32 scatter with K = 25 * Cs is a 94 %
                # padded MFMA tile: 494 us against ~60 us at 32 images of 128 x 128)
                dyp = torch.zeros((B, H, W, 8), dtype=torch.float32, device=dy.device)
                dyp[..., :Co] = dy.permute(0, 2, 3, 1)
                dx = ops.conv_scatter_bf16x3(ops.split_f32(dyp), (B, 8, H, W), ops.pack_w5_p1_split_padded(weight, 8), Ci, 5, 1, H, W)
            elif r.dx == "smallout_flipped":
                # input gradient of a stride-1 first conv (the VAE-GAN discriminator's 1 -> 32, models/networks.py:160-163:
                # its input is the decoder's output): dx[p] = sum_{tap, co} dy[p - tap + 2][co] W[co][ci][tap] is the
                # "many channels -> 1 | 3" correlation of the tap-in-N kernel with the taps flipped
                wf = weight.flip(2, 3).permute(1, 2, 3, 0).reshape(Ci, 25, Co).contiguous()      # [ci][tap'][co]
                dx = ops.conv5_smallout_bf16x3(dy, wf, None, ACT_NONE)
            elif r.dx == "scatter_padded":
                # the image side of a FIRST conv whose input gradient is needed (the VAE-GAN discriminator's, models/
                # networks.py:160-163: its input is the decoder's output): zero-pad the weight's input channels to 8,
                # scatter on the split-bf16 kernels, keep the real channels.  The exact-f32 scatter to one output channel
                # pads the MFMA tile's 32 columns by 97 %: 522 us against 32 + 214 us at 48 images of 128 x 128
                # (tools/microbench_narrow_dgrad.py)
                _, p1 = ops.pack_w_split(_pad_w(weight, Co, 8), False, True)
                dx = ops.conv_scatter_bf16x3(ops.split_f32(dy), sshape, p1, 8, ks, stride, H, W)[:, :Ci]
            else:               # "padded" | "x16" | "f32"
                dx = _scatter(dy if r.dx == "f32" else dys, sshape, _pad_w(weight, Cop, Cip), None, stride, H, W)
                dx = dx[:, :Ci] if Cip != Ci else dx
        if need_dw and dw is None:
            if r.dw == "smallout_wgrad":
                dw = ops.conv5_smallout_wgrad_bf16x3(a, dy, out=_grad_out(weight))
            elif r.dw == "padded":
                dw = _wgrad(a, (B, Cip, H, W), dys, sshape, ks, stride)[:Co, :Ci].contiguous()
            else:               # "x16" | "f32"
                dw = _wgrad(a, ctx.xshape, dy if r.dw == "f32" else dys, sshape, ks, stride, weight)
        if ctx.bias_param is not None and need_db:
            db = _bias_grad(dy, ctx.bias_param)
        return dx, dw, db, None, None, None


class _ConvT(Function):
    """big = bias + convT(small) with Hb = stride * Hs: kernel 5, padding 2, output_padding stride - 1 (models/networks.py:38) or
    kernel 4, stride 2, padding 1 (models/network_Style_GAN.py:49,116); weight (Csmall, Cbig, k, k) = nn.ConvTranspose2d layout
    (in_channels first).  The bias is added in the scatter kernel's epilogue."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride: int):
        x = _cl(x)
        B, Cs, Hs, Ws = x.shape
        ctx.route = _convt_route(_PRECISION, Cs, weight.shape[1])
        a = _split_of(x) if ctx.route == "x16" else x          # the split copy is what the weight gradient reads
        y = _scatter(a, x.shape, weight, bias, stride, Hs * stride, Ws * stride)
        ctx.stride, ctx.xshape = stride, tuple(x.shape)
        ctx.bias_param = bias
        ctx.save_for_backward(a, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, weight = ctx.saved_tensors
        dy = _cl(dy)
        dx = dw = db = None
        dys = _split_of(dy) if ctx.route == "x16" else dy
        if ctx.needs_input_grad[0]:
            dx = _gather(dys, dy.shape, weight, None, ctx.stride)
        if ctx.needs_input_grad[1]:
            dw = _wgrad(dys, tuple(dy.shape), a, ctx.xshape, weight.shape[2], ctx.stride, weight)
        if ctx.bias_param is not None and ctx.needs_input_grad[2]:
            db = _bias_grad(dy, ctx.bias_param)
        return dx, dw, db, None


class _BatchNormAct(Function):
    """y = act(BN(x)); x is (B,C,H,W) channels_last or (B,F).  Training mode uses batch statistics
    and updates the running buffers in place with torch's momentum semantics."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training: bool, momentum: float, eps: float,
                act: int, slope: float):
        x = _cl(x) if x.dim() == 4 else x.contiguous()
        if training:
            mean, rstd = ops.bn_stats(x, eps, momentum, running_mean, running_var)
        else:
            mean = running_mean
            rstd = torch.rsqrt(running_var + eps)
        if _PRECISION == "bf16x3" and x.dim() == 4 and x.shape[1] % 8 == 0:
            # the consumer is almost always a convolution on the split-bf16 kernels: emit its operand planes from this pass
            y, ys = ops.bn_act_fwd(x, mean, rstd, gamma, beta, act, slope, want_split=True)
            y._vp_split = (ys, y._version)
        else:
            y = ops.bn_act_fwd(x, mean, rstd, gamma, beta, act, slope)
        ctx.act, ctx.slope, ctx.training = act, slope, training
        ctx.save_for_backward(x, mean, rstd, gamma, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        dy = _cl(dy) if dy.dim() == 4 else dy.contiguous()
        need_affine = gamma is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        og = _grad_out(gamma) if (need_affine and ctx.needs_input_grad[1]) else None
        ob = _grad_out(beta) if (need_affine and ctx.needs_input_grad[2]) else None
        if _PRECISION == "bf16x3" and _BWD_SPLIT and x.dim() == 4 and x.shape[1] % 8 == 0 and ctx.needs_input_grad[0]:
            # dx is almost always the output gradient of a convolution on the split-bf16 kernels: emit its operand planes from
            # this pass (the tensor object travels through the autograd engine with its attribute; _split_of checks the version)
            dx, dgamma, dbeta, dxs = ops.bn_act_bwd(x, dy, mean, rstd, gamma, beta, ctx.act, ctx.slope, ctx.training, need_affine,
                                                    out_dgamma=og, out_dbeta=ob, want_split=True)
            dx._vp_split = (dxs, dx._version)
        else:
            dx, dgamma, dbeta = ops.bn_act_bwd(x, dy, mean, rstd, gamma, beta, ctx.act, ctx.slope, ctx.training, need_affine,
                                               out_dgamma=og, out_dbeta=ob)
        return dx, dgamma, dbeta, None, None, None, None, None, None, None


class _Linear(Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        y = ops.linear_fwd(x, weight, bias)
        ctx.has_bias = bias is not None
        ctx.bias_param = bias
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.linear_dgrad(dy, weight)
        if ctx.needs_input_grad[1]:
            dw = ops.linear_wgrad(dy, x, out=_grad_out(weight))
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = ops.colsum(dy, out=_grad_out(ctx.bias_param))
        return dx, dw, db


class _FlattenNCHW(Function):
    """(B,C,H,W) channels_last -> (B, C*H*W) in the reference's (C,H,W) flatten order
    (``ten.view(len(ten), -1)``, models/networks.py:74) via the HIP transpose."""

    @staticmethod
    def forward(ctx, x):
        x = _cl(x)
        ctx.shape = x.shape
        return ops.nhwc_to_nchw(x).reshape(x.shape[0], -1)

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W = ctx.shape
        return ops.nchw_to_nhwc(dy.contiguous().view(B, C, H, W))


class _UnflattenNCHW(Function):
    """(B, C*H*W) -> (B,C,H,W) channels_last (``ten.view(len(ten), -1, 8, 8)``, models/networks.py:110)."""

    @staticmethod
    def forward(ctx, x, C: int, H: int, W: int):
        B = x.shape[0]
        return ops.nchw_to_nhwc(x.contiguous().view(B, C, H, W))

    @staticmethod
    def backward(ctx, dy):
        dy = _cl(dy)
        return ops.nhwc_to_nchw(dy).reshape(dy.shape[0], -1), None, None, None


class _Act(Function):
    """Standalone activation (conv + bias + act blocks with bn=None, models/blocks.py:24-30)."""

    @staticmethod
    def forward(ctx, x, act: int, slope: float):
        if x.dim() != 4:
            x = x.contiguous()      # (a view with gaps, e.g. the flattened channel slice of a padded convolution output: the kernel walks dense memory)
        y = ops.act_fwd(x if (x.dim() != 4 or ops._is_nhwc(x)) else _cl(x), act, slope)
        ctx.act, ctx.slope = act, slope
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _cl(dy) if dy.dim() == 4 else dy.contiguous()
        return ops.act_bwd_from_y(y, dy, ctx.act, ctx.slope), None, None


class _InstanceNormAct(Function):
    """nn.InstanceNorm2d (affine=False, no running stats, eps 1e-5) + activation: per-(image, channel) statistics, one
    batched launch sequence (the BatchNorm kernels with blockIdx.z = image)."""

    @staticmethod
    def forward(ctx, x, eps: float, act: int, slope: float):
        x = _cl(x)
        if _PRECISION == "bf16x3" and _BWD_SPLIT and x.shape[1] % 8 == 0:
            # as _BatchNormAct: the consumer is almost always a convolution on the split-bf16 kernels
            y, mean, rstd, ys = ops.instnorm_act_fwd(x, eps, act, slope, want_split=True)
            y._vp_split = (ys, y._version)
        else:
            y, mean, rstd = ops.instnorm_act_fwd(x, eps, act, slope)
        ctx.act, ctx.slope = act, slope
        ctx.save_for_backward(x, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        if _PRECISION == "bf16x3" and _BWD_SPLIT and x.shape[1] % 8 == 0:
            dx, dxs = ops.instnorm_act_bwd(x, _cl(dy), mean, rstd, ctx.act, ctx.slope, want_split=True)
            dx._vp_split = (dxs, dx._version)
            return dx, None, None, None
        return ops.instnorm_act_bwd(x, _cl(dy), mean, rstd, ctx.act, ctx.slope), None, None, None


class _PairBlend(Function):
    """conv_1(x) * (1 - label) + conv_2(x) * label behind one stacked convolution (models/network_Style_GAN.py:72-79): u holds
    both branches along the channel, norm = InstanceNorm2d of each branch before the activation.  ``label`` (B,) is a constant."""

    @staticmethod
    def forward(ctx, u, label, norm: bool, eps: float, act: int, slope: float):
        u = _cl(u)
        C = u.shape[1] // 2
        ctx.split = _PRECISION == "bf16x3" and _BWD_SPLIT and C % 8 == 0       # as _InstanceNormAct
        y, mean, rstd, ys = ops.pair_blend_fwd(u, label, norm, eps, act, slope, want_split=ctx.split)
        if ys is not None:
            y._vp_split = (ys, y._version)
        ctx.norm, ctx.act, ctx.slope = norm, act, slope
        ctx.save_for_backward(u, label, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        u, label, mean, rstd = ctx.saved_tensors
        du, dus = ops.pair_blend_bwd(u, _cl(dy), label, mean, rstd, ctx.norm, ctx.act, ctx.slope, want_split=ctx.split)
        if dus is not None:
            du._vp_split = (dus, du._version)
        return du, None, None, None, None, None


class _Upsample2x(Function):
    """F.interpolate(scale_factor=2, mode='bilinear') -- models/blocks.py:145."""

    @staticmethod
    def forward(ctx, x):
        return ops.upsample2x_fwd(_cl(x))

    @staticmethod
    def backward(ctx, dy):
        return ops.upsample2x_bwd(_cl(dy))


class _AddCoords(Function):
    """AddCoords (models/blocks.py:97-112)."""

    @staticmethod
    def forward(ctx, x, normalize: bool):
        ctx.C = x.shape[1]
        return ops.add_coords(_cl(x), normalize)

    @staticmethod
    def backward(ctx, dy):
        return ops.slice_channels(_cl(dy), ctx.C), None


class _Reparam(Function):
    @staticmethod
    def forward(ctx, mu, logvar, eps):
        z, _ = ops.latent_fwd(mu, logvar, eps, want_kl=False)
        ctx.save_for_backward(mu, logvar, eps)
        return z

    @staticmethod
    def backward(ctx, dz):
        mu, logvar, eps = ctx.saved_tensors
        dmu, dlv = ops.latent_bwd(mu, logvar, eps, dz, None, 0.0)
        return dmu, dlv, None


class _KL(Function):
    """kl[b] = -0.5 * sum_j(1 + logvar - mu^2 - exp(logvar))."""

    @staticmethod
    def forward(ctx, mu, logvar):
        zeros = torch.zeros_like(mu)
        _, kl = ops.latent_fwd(mu, logvar, zeros, want_kl=True)
        ctx.save_for_backward(mu, logvar, zeros)
        return kl

    @staticmethod
    def backward(ctx, gkl):
        mu, logvar, zeros = ctx.saved_tensors
        dmu, dlv = ops.latent_bwd(mu, logvar, zeros, None, gkl, 0.0)
        return dmu, dlv


class _BCESum(Function):
    @staticmethod
    def forward(ctx, p, t):
        if p.dim() == 4:
            p, t = _cl(p), _cl(t)
        else:
            p, t = p.contiguous(), t.contiguous()
        out = ops.bce_sum(p, t)
        ctx.save_for_backward(p, t)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        return ops.bce_bwd(p, t, g.reshape(1).contiguous(), 1.0), None


class _GlobalAvgPool(Function):
    """nn.AdaptiveAvgPool2d((1, 1)) + flatten: (B, C, H, W) -> (B, C)."""

    @staticmethod
    def forward(ctx, x):
        x = _cl(x)
        ctx.shape = tuple(x.shape)
        return ops.global_avgpool_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        return ops.global_avgpool_bwd(dy.contiguous(), ctx.shape)


class _SCSE(Function):
    """SCSEBlock (models/blocks.py:52-65): y = x * cSE(x) + x * sSE(x) = x (c + s), optionally followed by a ReLU in the same
    store; fp32 whatever ``set_conv_precision`` says (no contraction here is worth an MFMA).  Backward needs x and the gates,
    never y: the fused ReLU's mask is x > 0, because c + s > 0."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, ws, bs, relu: bool):
        x = _cl(x)
        y, pool, hid, cgate, sgate = ops.scse_fwd(x, w1, b1, w2, b2, ws, bs, relu)
        if any(ctx.needs_input_grad):
            ctx.relu = relu
            ctx.params = (w1, b1, w2, b2, ws, bs)      # the Parameters themselves: _grad_out looks for their arena slices
            ctx.save_for_backward(x, w1, w2, ws, pool, hid, cgate, sgate)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2, ws, pool, hid, cgate, sgate = ctx.saved_tensors
        need = ctx.needs_input_grad
        # one kernel sequence produces all six parameter gradients; those that are wanted go straight into the arena where there is one
        out = [_grad_out(p) if need[i + 1] else None for i, p in enumerate(ctx.params)]
        dx, *grads = ops.scse_bwd(x, _cl(dy), w1, w2, ws, pool, hid, cgate, sgate, ctx.relu, need_dx=need[0], out=out)
        return (dx, *(g if need[i + 1] else None for i, g in enumerate(grads)), None)


class _TwinHead(Function):
    """The Style-GAN discriminator's output stage (models/network_Style_GAN.py:214-229): the two last 3x3 stride-2 convolutions on
    2 x 2 maps with their sigmoid and softmax, one launch forward and one backward; fp32 whatever ``set_conv_precision`` says
    (1 + K dot products per image are nothing for an MFMA)."""

    @staticmethod
    def forward(ctx, h_adv, h_aux, w_adv, b_adv, w_aux, b_aux):
        h_adv, h_aux = _cl(h_adv), _cl(h_aux)
        ctx.set_materialize_grads(False)                   # an output the loss does not use arrives as None: a null d_adv / d_aux
        adv, aux = ops.twin_head_fwd(h_adv, h_aux, w_adv, b_adv, w_aux, b_aux)
        if any(ctx.needs_input_grad):
            ctx.params = (w_adv, b_adv, w_aux, b_aux)      # the Parameters themselves: _grad_out looks for their arena slices
            ctx.save_for_backward(h_adv, h_aux, w_adv, w_aux, adv, aux)
        return adv, aux

    @staticmethod
    def backward(ctx, d_adv, d_aux):
        h_adv, h_aux, w_adv, w_aux, adv, aux = ctx.saved_tensors
        need = ctx.needs_input_grad
        out = [_grad_out(p) if need[i + 2] else None for i, p in enumerate(ctx.params)]
        dh_adv, dh_aux, *grads = ops.twin_head_bwd(h_adv, h_aux, w_adv, w_aux, adv, aux, d_adv, d_aux, out=out)
        return (dh_adv if need[0] else None, dh_aux if need[1] else None, *(g if need[i + 2] else None for i, g in enumerate(grads)))


class _SoftmaxRows(Function):
    """softmax over the last dimension of a 2-D tensor, on vp_softmax_rows_{fwd,bwd}_f32."""

    @staticmethod
    def forward(ctx, x):
        y = ops.softmax_rows_fwd(x.contiguous())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.softmax_rows_bwd(y, dy.contiguous())


class _SelfAttention(Function):
    """out = gamma * (V^T att^T) + x with att = softmax(Q K^T) per image (models/blocks.py:77-96); q, k, v are the
    already-projected (B, c', H, W) maps.  Per image: three HIP GEMMs + a row softmax; N = H*W = 1 (the only use in
    the font model, models/networks_BE_font.py:29-45) short-circuits to out = gamma * v + x."""

    @staticmethod
    def forward(ctx, x, q, k, v, gamma):
        x, q, k, v = _cl(x), _cl(q), _cl(k), _cl(v)
        B, C, H, W = x.shape
        N, C8 = H * W, q.shape[1]
        ctx.dims = (B, C, H, W, C8)
        if N == 1:
            att, o = None, v
        else:
            qm, km, vm = (t.permute(0, 2, 3, 1).reshape(B, N, -1) for t in (q, k, v))     # views of the NHWC memory
            att = torch.empty((B, N, N), dtype=torch.float32, device=x.device)
            o_m = torch.empty((B, N, C), dtype=torch.float32, device=x.device)
            for b in range(B):
                e = ops.gemm(qm[b], C8, 1, km[b], C8, 1, N, N, C8, 0)                    # energy = Q K^T
                att[b] = ops.softmax_rows_fwd(e)
                ops.gemm(att[b], N, 1, vm[b], 1, C, N, C, N, 1, out=o_m[b])              # out = att V
            o = o_m.view(B, H, W, C).permute(0, 3, 1, 2)
        ctx.save_for_backward(q, k, v, att, o, gamma)
        return gamma * o + x

    @staticmethod
    def backward(ctx, g):
        q, k, v, att, o, gamma = ctx.saved_tensors
        B, C, H, W, C8 = ctx.dims
        N = H * W
        g = _cl(g)
        dgamma = (g * o).sum().reshape(1)
        do = gamma * g
        if N == 1:
            return g, torch.zeros_like(q), torch.zeros_like(k), do, dgamma
        qm, km, vm = (t.permute(0, 2, 3, 1).reshape(B, N, -1) for t in (q, k, v))
        dom = _cl(do).permute(0, 2, 3, 1).reshape(B, N, C)
        dq, dk, dv = (torch.empty((B, N, n), dtype=torch.float32, device=g.device) for n in (C8, C8, C))
        for b in range(B):
            ops.gemm(att[b], 1, N, dom[b], 1, C, N, C, N, 2, out=dv[b])                  # dV = att^T dO
            datt = ops.gemm(dom[b], C, 1, vm[b], C, 1, N, N, C, 0)                       # dAtt = dO V^T
            de = ops.softmax_rows_bwd(att[b], datt)
            ops.gemm(de, N, 1, km[b], 1, C8, N, C8, N, 1, out=dq[b])                     # dQ = dE K
            ops.gemm(de, 1, N, qm[b], 1, C8, N, C8, N, 2, out=dk[b])                     # dK = dE^T Q
        to4 = lambda t, c: t.view(B, H, W, c).permute(0, 3, 1, 2)
        return g, to4(dq, C8), to4(dk, C8), to4(dv, C), dgamma


class _SelfAttentionFused(Function):
    """The same function as _SelfAttention for N = H*W > 1 on the flash-style kernels (csrc/attention.hip): one launch forward for
    the whole batch, at most five backward, and no (B, N, N) map: backward recomputes it from the per-row log-sum-exp.  Saves
    q, k, v, o, lse and gamma (o because gamma may be 0, so it cannot be had from the output)."""

    @staticmethod
    def forward(ctx, x, q, k, v, gamma):
        x, q, k, v = _cl(x), _cl(q), _cl(k), _cl(v)
        B, C, H, W = x.shape
        N, C8 = H * W, q.shape[1]
        ctx.dims = (B, C, H, W, C8)
        xm, qm, km, vm = (t.permute(0, 2, 3, 1).reshape(B, N, -1) for t in (x, q, k, v))      # views of the NHWC memory
        gamma = gamma.detach().reshape(1).contiguous()
        y, o, lse = ops.attention_fwd(qm, km, vm, xm, gamma)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(qm, km, vm, o, lse, gamma)
        return y.view(B, H, W, C).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        qm, km, vm, o, lse, gamma = ctx.saved_tensors
        B, C, H, W, C8 = ctx.dims
        need = ctx.needs_input_grad
        g = _cl(g)
        gm = g.permute(0, 2, 3, 1).reshape(B, H * W, C)
        dq, dk, dv, dgamma = ops.attention_bwd(qm, km, vm, o, lse, gm, gamma, need[1], need[2], need[3])
        to4 = lambda t, c: None if t is None else t.view(B, H, W, c).permute(0, 3, 1, 2)
        return g if need[0] else None, to4(dq, C8), to4(dk, C8), to4(dv, C), dgamma if need[4] else None


_ATTENTION_ROUTE = "auto"


def set_attention_route(route: str) -> None:
    """Which kernels run ``self_attention`` for N = H*W > 1: "fused" (the flash-style kernels, no N x N map), "gemm" (per image
    three GEMMs and a row softmax, the map kept for backward) or "auto" (the default: attention_route_for).  Both are exact fp32;
    ``set_conv_precision`` does not reach either.  N = 1 short-circuits on every route."""
    global _ATTENTION_ROUTE
    if route not in ("auto", "fused", "gemm"):
        raise ValueError("attention route must be 'auto', 'fused' or 'gemm'")
    _ATTENTION_ROUTE = route


def get_attention_route() -> str:
    return _ATTENTION_ROUTE


def attention_route_for(B: int, N: int, dq: int, C: int) -> str:
    """What "auto" resolves to, a pure host function of the shape: "gemm" at N = 1 (the short-circuit lives there), else the route
    whose forward + backward is estimated faster by the two-term model fitted to the measured table of DESIGN.md section 11.2
    (profiles/r12_attention.json; the model reproduces all nine measured shapes' winners):
      fused  its workgroups walk N/64 swept tiles, each a chain of 32-column contraction steps at ~1.4 us per step: dK and dQ
             (C/32 + dq/32 + 2 steps each) and forward and dV (dq/32 + 2 steps each); longer by B * N/64 / 512 once the
             workgroups no longer fit the chip at once;
      gemm   8 entry-point calls per image at ~11.6 us each, or 6 (C + dq) N^2 B flops at ~40 TF/s, whichever is larger.
    So "fused" where the GEMM route is launch-bound (many images, short sweeps: RefineNet's (16, 258, 32, 256), 7x faster) and
    "gemm" where few images do much work each (ValueEncoder's (4, 2048, 90, 720): the fused backward takes 2x the time there and
    is chosen only by ``set_attention_route("fused")``, for its memory: no (B, N, N) map)."""
    if N == 1:
        return "gemm"
    tiles, ns, nc = -(-N // 64), -(-dq // 32), -(-C // 32)
    fused_us = 1.4 * tiles * (2 * (nc + ns + 2) + 2 * (ns + 2)) * max(1.0, B * tiles / 512.0)
    gemm_us = max(11.6 * 8 * B, 6.0 * (C + dq) * N * N * B / 40e6)
    return "fused" if fused_us <= gemm_us else "gemm"


class _L1Mean(Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        ctx.save_for_backward(a, b)
        return ops.l1_mean(a, b).reshape(())

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da, db = ops.l1_mean_bwd(a, b, g.reshape(1).contiguous(), ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return da, db


class _CrossEntropy(Function):
    """F.cross_entropy(logits, labels) with torch's defaults (mean), on vp_cross_entropy_{fwd,bwd}_f32."""

    @staticmethod
    def forward(ctx, logits, labels):
        loss, prob = ops.cross_entropy_fwd(logits.contiguous(), labels.contiguous())
        ctx.save_for_backward(prob, labels)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        prob, labels = ctx.saved_tensors
        return ops.cross_entropy_bwd(prob, labels.contiguous(), g.reshape(1).contiguous()), None


class _BELoss(Function):
    """bce_weight * BCEWithLogits(x, t) (mean) + dice(sigmoid(x), t) as one reduction + one elementwise backward."""

    @staticmethod
    def forward(ctx, logits, targets, bce_weight: float, smooth: float):
        logits, targets = logits.contiguous(), targets.contiguous()
        loss, sums = ops.be_loss_fwd(logits, targets, bce_weight, smooth)
        ctx.w, ctx.smooth = bce_weight, smooth
        ctx.save_for_backward(logits, targets, sums)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        logits, targets, sums = ctx.saved_tensors
        return ops.be_loss_bwd(logits, targets, sums, g.reshape(1).contiguous(), ctx.w, ctx.smooth), None, None, None


class _DiceLoss(Function):
    """1 - mean_b (2 sum(p t) + s) / (sum p + sum t + s) on probabilities (no gradient to the targets)."""

    @staticmethod
    def forward(ctx, probs, targets, smooth: float):
        probs, targets = probs.contiguous(), targets.contiguous()
        loss, sums = ops.dice_loss_fwd(probs, targets, smooth)
        ctx.smooth = smooth
        ctx.save_for_backward(probs, targets, sums)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        probs, targets, sums = ctx.saved_tensors
        return ops.dice_loss_bwd(probs, targets, sums, g.reshape(1).contiguous(), ctx.smooth), None, None


class _HalfSqDiff(Function):
    """0.5*(a-b)^2 per element ("nle", models/networks.py:267) or summed over all but the first dim (":273")."""

    @staticmethod
    def forward(ctx, a, b, rowsum: bool):
        a, b = a.contiguous(), b.contiguous()
        ctx.rowsum = rowsum
        ctx.save_for_backward(a, b)
        return ops.half_sqdiff_rowsum(a, b) if rowsum else ops.half_sqdiff(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da, db = ops.half_sqdiff_bwd(a, b, g.contiguous(), ctx.rowsum, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return da, db, None


# ---- public functional API ----------------------------------------------------------------------
def conv5x5(x, weight, bias=None, stride: int = 2, act: Optional[str] = None):
    if tuple(weight.shape[2:]) != (5, 5):
        raise ValueError("conv5x5 takes a (Cout, Cin, 5, 5) weight")
    return _Conv.apply(x, weight, bias, stride, ACT_CODES[act], "conv5x5")


def conv_transpose5x5(x, weight, stride: int = 2):
    return _ConvT.apply(x, weight, None, stride)


def batch_norm_act(x, gamma, beta, running_mean, running_var, training: bool, momentum: float = 0.1, eps: float = 1e-5,
                   act: Optional[str] = "relu", slope: float = 0.0):
    return _BatchNormAct.apply(x, gamma, beta, running_mean, running_var, training, momentum, eps, ACT_CODES[act], slope)


def linear(x, weight, bias=None):
    return _Linear.apply(x, weight, bias)


def conv2d(x, weight, bias=None, stride: int = 1):
    """k x k convolution, k in {1,3,4,5}, padding (k-1)//2 (models/blocks.py Conv2d)."""
    return _Conv.apply(x, weight, bias, stride, ACT_NONE, "conv2d")


def conv_transpose2d(x, weight, bias=None, stride: int = 2):
    """nn.ConvTranspose2d(in, out, 4, 2, 1) (models/network_Style_GAN.py:49,116): weight (in, out, 4, 4), output 2H x 2W."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (4, 4) or stride != 2:
        raise ValueError("HIP conv_transpose2d supports kernel_size 4, stride 2, padding 1")
    return _ConvT.apply(x, weight, bias, stride)


def activation(x, act: Optional[str], slope: float = 0.0):
    code = ACT_CODES[act]
    return x if code == ACT_NONE else _Act.apply(x, code, slope)


def instance_norm_act(x, eps: float = 1e-5, act: Optional[str] = None, slope: float = 0.0):
    return _InstanceNormAct.apply(x, eps, ACT_CODES[act], slope)


def pair_blend(u, label, norm: bool = False, eps: float = 1e-5, act: Optional[str] = None, slope: float = 0.0):
    """Label-gated blend of the two halves of ``u`` (B, 2C, H, W) -> (B, C, H, W): (1 - label[b]) * act(n(u[:, :C])) +
    label[b] * act(n(u[:, C:])), n = InstanceNorm2d(eps) with ``norm`` else the identity.  ``label``: B elements of any dtype,
    a constant (no gradient)."""
    if u.dim() != 4 or u.shape[1] % 2 != 0 or label.numel() != u.shape[0]:
        raise ValueError("pair_blend: u must be (B, 2C, H, W) and label must have B elements")
    label = label.detach().reshape(-1).to(device=u.device, dtype=torch.float32).contiguous()
    return _PairBlend.apply(u, label, bool(norm), eps, ACT_CODES[act], slope)


def upsample2x_bilinear(x):
    return _Upsample2x.apply(x)


def add_coords(x, normalize: bool = False):
    return _AddCoords.apply(x, normalize)


def flatten_nchw(x):
    return _FlattenNCHW.apply(x)


def unflatten_nchw(x, C: int, H: int, W: int):
    return _UnflattenNCHW.apply(x, C, H, W)


def reparameterize(mu, logvar, *, eps: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None):
    """z = eps * exp(0.5*logvar) + mu (models/networks.py:228-231).  The reference draws eps with
    ``normal_()``; here it may be injected (parity tests) or drawn with torch's device RNG."""
    if eps is None:
        eps = torch.randn(mu.shape, dtype=mu.dtype, device=mu.device, generator=generator)
    return _Reparam.apply(mu, logvar, eps)


def kl_divergence(mu, logvar):
    """Per-sample KL of models/networks.py:270, shape (B,)."""
    return _KL.apply(mu, logvar)


def binary_cross_entropy(p, t, reduction: str = "sum"):
    """F.binary_cross_entropy with torch's -100 log clamp; reduction 'sum' or 'mean'."""
    s = _BCESum.apply(p, t)
    if reduction == "sum":
        return s
    if reduction == "mean":
        return s / p.numel()
    raise ValueError("reduction must be 'sum' or 'mean'")


def global_avg_pool(x):
    """nn.AdaptiveAvgPool2d((1, 1)) followed by the flatten of models/networks_BE_font.py:66: (B, C, H, W) -> (B, C)."""
    return _GlobalAvgPool.apply(x)


def scse(x, w1, b1, w2, b2, ws, bs, relu: bool = False):
    """SCSEBlock.forward (models/blocks.py:64-65) on the block's six parameters (cSE.1, cSE.3, sSE.0 weight and bias);
    ``relu=True`` also applies the ReLU that follows two of these blocks in StyleUp.cat_convs (models/network_Style_GAN.py:54-59)."""
    return _SCSE.apply(x, w1, b1, w2, b2, ws, bs, bool(relu))


def twin_head(h_adv, h_aux, w_adv, b_adv, w_aux, b_aux):
    """The Style-GAN discriminator's output stage (models/network_Style_GAN.py:214-229) on the (B, C, 2, 2) outputs of adv_convs.0 and
    aux_convs.0: (adv_res (B, 1), aux_res (B, K)) = (sigmoid, softmax) of the 3x3 stride-2 convolutions with w_adv (1, C, 3, 3) and
    w_aux (K, C, 3, 3), as one kernel forward and one backward."""
    return _TwinHead.apply(h_adv, h_aux, w_adv, b_adv, w_aux, b_aux)


def softmax_rows(x2d):
    """``x2d.softmax(dim=-1)`` of a 2-D tensor."""
    if x2d.dim() != 2:
        raise ValueError("softmax_rows: a 2-D tensor is expected")
    return _SoftmaxRows.apply(x2d)


def self_attention(x, q, k, v, gamma):
    """SelfAttentionBlock's core on the already-projected maps: gamma * softmax(q k^T) v + x per image (models/blocks.py:77-96),
    on the route ``set_attention_route`` names."""
    B, C, H, W = x.shape
    route = _ATTENTION_ROUTE
    if route == "auto":
        route = attention_route_for(B, H * W, q.shape[1], C)
    if H * W == 1 or route == "gemm":
        return _SelfAttention.apply(x, q, k, v, gamma)
    return _SelfAttentionFused.apply(x, q, k, v, gamma)


def cross_entropy(logits, labels):
    """``F.cross_entropy(logits, labels)`` for (B, classes) logits and int64 class indices (train_BE_GAN.py:135,159: the
    discriminator's type losses; train_BE_font.py:109): a HIP kernel, like every other loss of the steps."""
    return _CrossEntropy.apply(logits, labels)


def l1_loss(a, b):
    """F.l1_loss(a, b) (mean)."""
    return _L1Mean.apply(a, b)


def be_loss(logits, targets, bce_weight: float = 0.5, smooth: float = 1.0):
    """train_BE.py:58-59: ``bce_weight * F.binary_cross_entropy_with_logits(logits, targets)
    + compute_dice_loss(logits.sigmoid(), targets)`` (tools/ops.py:12-19) for (B, ...) logits; scalar."""
    return _BELoss.apply(logits, targets, bce_weight, smooth)


def dice_loss(probs, targets, smooth: float = 1.0):
    """tools/ops.py:12-19 / :178-185 on probabilities."""
    return _DiceLoss.apply(probs, targets, smooth)


_EDGE_KERNEL = None


def edge_loss(mask_probs, mask_targets):
    """tools/ops.py:187-215: dice loss between |Laplacian| edge maps of prediction and target (single-channel maps;
    3x3 kernel [[-1,-1,-1],[-1,8,-1],[-1,-1,-1]] / 8, zero padding).  The filter is a fixed-weight 3x3 convolution on the
    HIP conv kernel; |e| = relu(e) + relu(-e) (the activation kernels differentiate through their OUTPUT, so an
    even function has to be assembled from monotone pieces)."""
    global _EDGE_KERNEL
    if _EDGE_KERNEL is None or _EDGE_KERNEL.device != mask_probs.device:
        k = torch.full((3, 3), -1.0)
        k[1, 1] = 8.0
        _EDGE_KERNEL = (k / 8).reshape(1, 1, 3, 3).to(mask_probs.device)
    def absmap(x):
        e = conv2d(x, _EDGE_KERNEL, None, 1)
        return activation(e, "relu") + activation(-e, "relu")

    return dice_loss(absmap(mask_probs), absmap(mask_targets).detach())


def half_sq_diff(a, b):
    """0.5 * (a - b) ** 2, elementwise."""
    return _HalfSqDiff.apply(a, b, False)


def half_sq_diff_rowsum(a, b):
    """torch.sum(0.5 * (a - b) ** 2, 1) for 2-D a, b."""
    return _HalfSqDiff.apply(a, b, True)


def vae_loss(x, x_tilde, mu, logvar):
    """(sum-BCE + sum-KL) / B -- the composed loss of SURVEY.md 3.3.  Returns (loss, recon, kl)."""
    recon = binary_cross_entropy(x_tilde, x, "sum")
    kl = kl_divergence(mu, logvar).sum()
    return (recon + kl) / x.shape[0], recon, kl
