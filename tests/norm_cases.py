"""What tests/test_gpu_norm_edges.py and tools/ab_norm_bits.py share: the shapes at which csrc/bn.hip's grids, trips and kernels change,
and every entry point of that file called on guarded buffers (tests/guarded.py) with an exact-size workspace.

The shapes come from bn_grid (1024 chunks of >= 64 rows), bn_apply_grid (4096 chunks of >= 64 rows), the 64-row trip of the row walk
(4 rows of 16) and the 64-channel block."""
import ctypes

import torch

TILED = [(1, 4), (17, 8), (63, 60), (64, 64), (65, 68), (129, 132), (200, 12)]     # edges of the 64-row trip and the 64-channel block
FLAT = [(16, 1), (70, 3), (130, 66)]                                               # the C % 4 != 0 kernels
FINALISER = [(8300, 8)]           # 130 row chunks: the finaliser's two-chain loop and its one-chain tail both run
REDUCTION_CAP = [(70000, 4)]      # the reduction grid at its 1024 cap: 69 rows per chunk, one full trip plus a 5-row tail
APPLY_CAP = [(262200, 4)]         # the apply grid at its 4096 cap: 65 rows per chunk
SMALL = [(32, 1024), (4, 32768), (64, 72), (7, 8), (1, 64)]                        # the one-launch BatchNorm (R <= 64, C % 4 == 0)
BN_SHAPES = TILED + FLAT + FINALISER + REDUCTION_CAP + APPLY_CAP + SMALL
BATCHED = [(B, R, C) for B in (1, 3) for R in (17, 65, 200) for C in (8, 68, 6)]   # InstanceNorm and pair blend
ACTS = (0, 1, 2, 3, 4)            # none, relu, leaky relu, tanh, sigmoid (VP_ACT_*)
SLOPE = 0.2
EPS = 1e-5


class Lib:
    """A library handle with _lib.SIGNATURES applied; call() raises on a non-zero status."""

    def __init__(self, path=None):
        from vae_play_amd import _lib
        self.h = _lib.load() if path is None else ctypes.CDLL(path)
        if path is not None:
            for name, (res, args) in _lib.SIGNATURES.items():
                if hasattr(self.h, name):
                    fn = getattr(self.h, name)
                    fn.restype, fn.argtypes = res, args

    def call(self, name, *args):
        rc = getattr(self.h, name)(*args)
        if rc != 0:
            raise RuntimeError(f"{name} failed (status {rc}): {(self.h.vp_last_error() or b'').decode()}")


OFFSET_BATCHED = [(3, 65, 68), (3, 200, 6)]   # InstanceNorm with inputs(..., offset=OFFSET): every image far from the others
OFFSET = 300.0


def inputs(B, R, C, seed=0, offset=0.0, device="cuda"):
    """x [B][R][C] with |mean| >> sigma per channel, dy, gamma, beta [C], label [B], on the device.  offset adds offset * randn per
    image and channel to x, drawn after everything else: a statistic, pivot or slab taken from another image is then far off."""
    g = torch.Generator().manual_seed(seed * 1000003 + B * 7919 + R * 131 + C)
    x = torch.randn(B, R, C, generator=g) * 1.5 + torch.randn(1, 1, C, generator=g) * 20
    dy = torch.randn(B, R, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    label = torch.rand(B, generator=g)
    if offset:
        x = x + offset * torch.randn(B, 1, C, generator=g)
    return [t.to(device) for t in (x, dy, gamma, beta, label)]


def _ps():
    from vae_play_amd import ops
    return ops._p, ops._pv, ops._stream()


def bn_stats(L, G, x, R, C, running=False, momentum=0.1):
    """-> mean, rstd, running_mean, running_var (the last two None unless running)"""
    P, _, st = _ps()
    mean, rstd = G.out("mean", C), G.out("rstd", C)
    rm = G.state("running_mean", torch.linspace(-1, 1, C)) if running else None
    rv = G.state("running_var", torch.linspace(0.5, 2, C)) if running else None
    ws, nb = G.ws("ws", L.h.vp_bn_workspace_bytes(R, C))
    L.call("vp_bn_stats_f32", P(x), R, C, EPS, momentum, P(mean), P(rstd), P(rm), P(rv), P(ws), nb, st)
    return mean, rstd, rm, rv


def bn_fwd(L, G, kind, x, mean, rstd, gamma, beta, R, C, act, fmt=0):
    """kind: plain | split | planes (y null) | fmt  -> y, planes (None where not asked for)"""
    P, PV, st = _ps()
    y = None if kind == "planes" else G.out("y", R, C)
    ys = None if kind == "plain" else G.planes("y_split", R * C)
    head = (P(x), P(mean), P(rstd), P(gamma), P(beta), P(y))
    if kind == "plain":
        L.call("vp_bn_act_fwd_f32", *head, R, C, act, SLOPE, st)
    elif kind == "fmt":
        L.call("vp_bn_act_fwd_split_fmt_f32", *head, PV(ys), R, C, act, SLOPE, fmt, st)
    else:
        L.call("vp_bn_act_fwd_split_f32", *head, PV(ys), R, C, act, SLOPE, st)
    return y, ys


def bn_bwd(L, G, kind, x, dy, mean, rstd, gamma, beta, R, C, act, batch_stats=1, affine_grads=True, fmt=0, scale=1.0):
    """kind: plain | split | planes (dx null) | fmt | sat  -> dx, planes, dgamma, dbeta, saturation flag (None where not asked for)"""
    P, PV, st = _ps()
    dx = None if kind == "planes" else G.out("dx", R, C)
    ds = None if kind == "plain" else G.planes("dx_split", R * C)
    dg, db = (G.out("dgamma", C), G.out("dbeta", C)) if affine_grads else (None, None)
    sat = G.state("saturated", torch.zeros(1)) if kind == "sat" else None      # an int32 0
    ws, nb = G.ws("ws", L.h.vp_bn_workspace_bytes(R, C))
    head = (P(x), P(dy), P(mean), P(rstd), P(gamma), P(beta), P(dx))
    tail = (P(dg), P(db), R, C, act, SLOPE, batch_stats)
    if kind == "plain":
        L.call("vp_bn_act_bwd_f32", *head, *tail, P(ws), nb, st)
    elif kind == "fmt":
        L.call("vp_bn_act_bwd_split_fmt_f32", *head, PV(ds), *tail, fmt, scale, P(ws), nb, st)
    elif kind == "sat":
        L.call("vp_bn_act_bwd_split_fmt_sat_f32", *head, PV(ds), *tail, fmt, scale, P(sat), P(ws), nb, st)
    else:
        L.call("vp_bn_act_bwd_split_f32", *head, PV(ds), *tail, P(ws), nb, st)
    return dx, ds, dg, db, (None if sat is None else sat.view(torch.int32))


def bn_small_fwd(L, G, x, gamma, beta, R, C, act, running=False, momentum=0.1):
    P, _, st = _ps()
    mean, rstd, y = G.out("mean", C), G.out("rstd", C), G.out("y", R, C)
    rm = G.state("running_mean", torch.linspace(-1, 1, C)) if running else None
    rv = G.state("running_var", torch.linspace(0.5, 2, C)) if running else None
    L.call("vp_bn_small_fwd_f32", P(x), R, C, EPS, momentum, P(gamma), P(beta), P(mean), P(rstd), P(rm), P(rv), P(y), act, SLOPE, st)
    return y, mean, rstd, rm, rv


def bn_small_bwd(L, G, x, dy, mean, rstd, gamma, beta, R, C, act, batch_stats=1):
    P, _, st = _ps()
    dx, dg, db = G.out("dx", R, C), G.out("dgamma", C), G.out("dbeta", C)
    L.call("vp_bn_small_bwd_f32", P(x), P(dy), P(mean), P(rstd), P(gamma), P(beta), P(dx), P(dg), P(db), R, C, act, SLOPE, batch_stats, st)
    return dx, dg, db


def act_fwd_bwd(L, G, x, dy, act):
    """vp_act_fwd_f32, then vp_act_bwd_from_y_f32 on its output -> y, dx"""
    P, _, st = _ps()
    y, dx = G.out("act_y", x.numel()), G.out("act_dx", x.numel())
    L.call("vp_act_fwd_f32", P(x), P(y), x.numel(), act, SLOPE, st)
    L.call("vp_act_bwd_from_y_f32", P(y), P(dy), P(dx), x.numel(), act, SLOPE, st)
    return y, dx


def inorm_fwd(L, G, x, B, R, C, act, split=False):
    """-> y, mean [B][C], rstd [B][C], planes"""
    P, PV, st = _ps()
    y, mean, rstd = G.out("y", B, R, C), G.out("mean", B, C), G.out("rstd", B, C)
    ys = G.planes("y_split", B * R * C) if split else None
    ws, nb = G.ws("ws", L.h.vp_instnorm_workspace_bytes(B, R, C))
    if split:
        L.call("vp_instnorm_act_fwd_split_f32", P(x), P(y), PV(ys), P(mean), P(rstd), B, R, C, EPS, act, SLOPE, P(ws), nb, st)
    else:
        L.call("vp_instnorm_act_fwd_f32", P(x), P(y), P(mean), P(rstd), B, R, C, EPS, act, SLOPE, P(ws), nb, st)
    return y, mean, rstd, ys


def inorm_fwd_ld(L, G, x, B, R, C, act, ldy, col):
    """y as columns [col, col + C) of a NaN-filled [B][R][ldy] buffer -> the whole buffer, mean [B][C], rstd [B][C]"""
    P, _, st = _ps()
    wide = G.ws("y_wide", B * R * ldy * 4)[0].view(B, R, ldy)          # the columns outside the slice keep their NaN
    mean, rstd = G.out("mean", B, C), G.out("rstd", B, C)
    ws, nb = G.ws("ws", L.h.vp_instnorm_workspace_bytes(B, R, C))
    L.call("vp_instnorm_act_fwd_ld_f32", P(x), P(wide[0, 0, col:]), ldy, P(mean), P(rstd), B, R, C, EPS, act, SLOPE, P(ws), nb, st)
    return wide, mean, rstd


def inorm_bwd(L, G, x, dy, mean, rstd, B, R, C, act, split=False):
    """-> dx, planes"""
    P, PV, st = _ps()
    dx = G.out("dx", B, R, C)
    ds = G.planes("dx_split", B * R * C) if split else None
    ws, nb = G.ws("ws", L.h.vp_instnorm_workspace_bytes(B, R, C))
    if split:
        L.call("vp_instnorm_act_bwd_split_f32", P(x), P(dy), P(mean), P(rstd), P(dx), PV(ds), B, R, C, act, SLOPE, P(ws), nb, st)
    else:
        L.call("vp_instnorm_act_bwd_f32", P(x), P(dy), P(mean), P(rstd), P(dx), B, R, C, act, SLOPE, P(ws), nb, st)
    return dx, ds


def pair_fwd(L, G, u, label, B, R, C, norm, act, split=False):
    """u [B][R][2C] -> y [B][R][C], mean, rstd [B][2C] (None when norm = 0), planes"""
    P, PV, st = _ps()
    y = G.out("y", B, R, C)
    mean, rstd = (G.out("mean", B, 2 * C), G.out("rstd", B, 2 * C)) if norm else (None, None)
    ys = G.planes("y_split", B * R * C) if split else None
    ws, nb = G.ws("ws", L.h.vp_pair_blend_workspace_bytes(B, R, C)) if norm else (None, 0)
    L.call("vp_pair_blend_fwd_f32", P(u), P(label), P(y), PV(ys), P(mean), P(rstd), B, R, C, norm, EPS, act, SLOPE, P(ws), nb, st)
    return y, mean, rstd, ys


def pair_bwd(L, G, u, dy, label, mean, rstd, B, R, C, norm, act, split=False):
    """dy [B][R][C] -> du [B][R][2C], planes"""
    P, PV, st = _ps()
    du = G.out("du", B, R, 2 * C)
    ds = G.planes("du_split", B * R * 2 * C) if split else None
    ws, nb = G.ws("ws", L.h.vp_pair_blend_workspace_bytes(B, R, C)) if norm else (None, 0)
    L.call("vp_pair_blend_bwd_f32", P(u), P(dy), P(label), P(mean), P(rstd), P(du), PV(ds), B, R, C, norm, act, SLOPE, P(ws), nb, st)
    return du, ds
