"""Record what the autograd convolution front end (functional.conv5x5 / conv_transpose5x5 / conv2d / conv_transpose2d) launches:
per case -- one layer, forward and backward, on tiny tensors -- the sequence of C-ABI calls with their scalar arguments and, per pointer
argument, "null", the name of the case's tensor that lives at the address (x, weight, bias, dy, y, dx, dw, db; "dw@arena" /
"db@arena" for a parameter's slice of an optim.FlatArena) or "tmp".  Only the public functional API is used; _lib.call and the
tensor-to-pointer helpers of ops are wrapped for the duration of a case, so the recorder runs unchanged on any revision of the front end: a refactor of functional.py
must reproduce the committed log (tests/golden/conv_frontend_launches.json, tests/test_gpu_conv_frontend_launches.py).

Entry names are canonicalised by three identities of the C side: vp_conv5_* is vp_conv_* with ks = 5, Hb = Hs * stride,
Wb = Ws * stride (csrc/conv.hip, csrc/conv16.hip), likewise vp_pack_w5_f32 / vp_pack_w5_split; vp_conv_scatter_bias_* with a null
bias is vp_conv_scatter_*.

usage: python tools/record_conv_launches.py [--out tests/golden/conv_frontend_launches.json] [--digests]
  --digests  also print a SHA-256 of y, dx, dw and db per case (bitwise comparison of two trees on ONE machine; never committed:
             the split-K depths follow the device)"""
import argparse
import contextlib
import ctypes
import hashlib
import json
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda"
B = 2


def _case(name, entry, mode, Cin, Cout, ks=5, stride=2, H=8, W=8, bias=False, act=None, feed="fresh", image_grad=True, flags=None,
          arena=False):
    return dict(name=name, entry=entry, mode=mode, Cin=Cin, Cout=Cout, ks=ks, stride=stride, H=H, W=W, bias=bias, act=act, feed=feed,
                image_grad=image_grad, flags=flags or {}, arena=arena)


def _both(name, entry, *a, **kw):
    return [_case(f"{name}-{m}", entry, m, *a, **kw) for m in ("f32", "bf16x3")]


# feed "bn": the input is a batch_norm_act output and dy a batch_norm_act input gradient, both carrying split planes in bf16x3 mode
CASES = [
    _case("conv5x5-8to16-s2-f32", "conv5x5", "f32", 8, 16),
    _case("conv5x5-64to1-s1-bias-sigmoid-f32", "conv5x5", "f32", 64, 1, stride=1, bias=True, act="sigmoid"),
    _case("conv5x5-8to16-s2-bf16x3", "conv5x5", "bf16x3", 8, 16),
    _case("conv5x5-8to16-s2-bn-bf16x3", "conv5x5", "bf16x3", 8, 16, feed="bn"),
    _case("conv5x5-1to8-s2-im2col-bf16x3", "conv5x5", "bf16x3", 1, 8),
    _case("conv5x5-1to8-s2-im2col-noimagegrad-bf16x3", "conv5x5", "bf16x3", 1, 8, image_grad=False),
    _case("conv5x5-3to8-s2-im2col-bf16x3", "conv5x5", "bf16x3", 3, 8),
    _case("conv5x5-3to8-s2-im2col-noimagegrad-bf16x3", "conv5x5", "bf16x3", 3, 8, image_grad=False),
    _case("conv5x5-1to32-s1-bias-relu-smallin-bf16x3", "conv5x5", "bf16x3", 1, 32, stride=1, bias=True, act="relu"),
    _case("conv5x5-64to1-s1-bias-sigmoid-smallout-bf16x3", "conv5x5", "bf16x3", 64, 1, stride=1, bias=True, act="sigmoid"),
    _case("conv5x5-64to3-s1-bias-sigmoid-smallout-bf16x3", "conv5x5", "bf16x3", 64, 3, stride=1, bias=True, act="sigmoid"),
    # 16 x 64: the smallest image the smallout weight-gradient kernel takes (height a multiple of 16, width of 64)
    _case("conv5x5-64to1-s1-bias-sigmoid-smallout-wgrad-16x64-bf16x3", "conv5x5", "bf16x3", 64, 1, stride=1, H=16, W=64, bias=True,
          act="sigmoid"),
    _case("conv5x5-16to3-s1-halo-padded-bf16x3", "conv5x5", "bf16x3", 16, 3, stride=1),
    _case("conv5x5-3to16-s1-scatter-padded-bf16x3", "conv5x5", "bf16x3", 3, 16, stride=1),
    _case("conv5x5-2to8-s2-bias-scatter-padded-bf16x3", "conv5x5", "bf16x3", 2, 8, bias=True),
    *_both("convT5-16to8-s2", "conv_transpose5x5", 16, 8),
    _case("convT5-16to3-s2-bf16x3", "conv_transpose5x5", "bf16x3", 16, 3),
    *_both("convT2d-8to16-bias", "conv_transpose2d", 8, 16, ks=4, bias=True),
    *_both("convT2d-8to16", "conv_transpose2d", 8, 16, ks=4),
    _case("convT2d-4to4-bias-bf16x3", "conv_transpose2d", "bf16x3", 4, 4, ks=4, bias=True),
    *_both("conv2d-3x3-16to16-s1-bias", "conv2d", 16, 16, ks=3, stride=1, bias=True),
    *_both("conv2d-3x3-16to16-s2", "conv2d", 16, 16, ks=3, stride=2),
    *_both("conv2d-1x1-16to16", "conv2d", 16, 16, ks=1, stride=1, bias=True),
    *_both("conv2d-4x4-16to16-s2-9x7", "conv2d", 16, 16, ks=4, stride=2, H=9, W=7, bias=True),
    *_both("conv2d-5x5-16to16-s2-7x7", "conv2d", 16, 16, ks=5, stride=2, H=7, W=7),
    *_both("conv2d-3x3-8to4-small3", "conv2d", 8, 4, ks=3, stride=1, bias=True),
    *_both("conv2d-3x3-8to4-small3-wgrad-only", "conv2d", 8, 4, ks=3, stride=1, bias=True, flags={"_SMALL3_ALL": False}),
    *_both("conv2d-3x3-8to4-small3-off", "conv2d", 8, 4, ks=3, stride=1, bias=True, flags={"_SMALL3": False}),
    _case("conv2d-3x3-10to16-padded-in-bf16x3", "conv2d", "bf16x3", 10, 16, ks=3, stride=1, bias=True),
    _case("conv2d-1x1-16to1-padded-out-bf16x3", "conv2d", "bf16x3", 16, 1, ks=1, stride=1, bias=True),
    _case("conv2d-3x3-16to16-s1-bn-bf16x3", "conv2d", "bf16x3", 16, 16, ks=3, stride=1, bias=True, feed="bn"),
    _case("conv2d-3x3-16to16-s1-bn-nobwdsplit-bf16x3", "conv2d", "bf16x3", 16, 16, ks=3, stride=1, bias=True, feed="bn",
          flags={"_BWD_SPLIT": False}),
    _case("conv2d-3x3-10to16-padded-in-arena-bf16x3", "conv2d", "bf16x3", 10, 16, ks=3, stride=1, bias=True, arena=True),
    _case("conv5x5-8to16-s2-bias-arena-bf16x3", "conv5x5", "bf16x3", 8, 16, bias=True, arena=True),
]
CASE_NAMES = [c["name"] for c in CASES]

_SCALARS = (ctypes.c_int, ctypes.c_long, ctypes.c_size_t, ctypes.c_float)


@contextlib.contextmanager
def _recording(raw):
    """_lib.call wrapped: every call appends (entry name, [("s", scalar) | ("p", address or None), ...]) to ``raw``.  ops._p / ops._pv
    (tensor -> pointer argument) are wrapped too, to keep every tensor that a launch sees alive until the case ends: a freed
    temporary's address would otherwise come back as a later tensor's, and the names would follow the allocator, not the code."""
    from vae_play_amd import _lib, ops
    orig, keep = (_lib.call, ops._p, ops._pv), []

    def call(name, *args):
        types = _lib.SIGNATURES[name][1]
        raw.append((name, [("s", a) if t in _SCALARS else ("p", getattr(a, "value", a)) for a, t in zip(args, types)]))
        return orig[0](name, *args)

    def keeping(to_pointer):
        def f(t):
            keep.append(t)
            return to_pointer(t)
        return f

    _lib.call, ops._p, ops._pv = call, keeping(orig[1]), keeping(orig[2])
    try:
        yield
    finally:
        _lib.call, ops._p, ops._pv = orig


def canonical(name, args):
    """(name, args without the stream) -> the generic entry that the C side forwards to, see the module docstring"""
    if name in ("vp_pack_w5_f32", "vp_pack_w5_split"):
        return name.replace("_w5_", "_w_"), args + [5]
    m = re.fullmatch(r"vp_conv5_(gather|scatter|wgrad)_(f32|bf16x3)", name)
    if m:
        nptr = 4 if m[1] == "gather" else 3
        Bn, Hs, Ws, C1, C2, stride = args[nptr:nptr + 6]
        return f"vp_conv_{m[1]}_{m[2]}", args[:nptr] + [Bn, Hs, Ws, Hs * stride, Ws * stride, C1, C2, 5, stride] + args[nptr + 6:]
    m = re.fullmatch(r"vp_conv_scatter_bias_(f32|bf16x3)", name)
    if m and args[2] == "null":
        return f"vp_conv_scatter_{m[1]}", args[:2] + args[3:]
    return name, args


def _digest(t):
    return None if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(case, digests=False):
    """-> (log, digests or None); log = [[entry, [arg, ...]], ...] with the stream argument dropped"""
    from vae_play_amd import functional as F, optim
    c = case
    gen = torch.Generator(device=DEV).manual_seed(sum(map(ord, c["name"])))
    ks, Cin, Cout, H, W = c["ks"], c["Cin"], c["Cout"], c["H"], c["W"]
    transposed = c["entry"].startswith("conv_transpose")

    def nhwc(C, h, w):
        return torch.randn(B, h, w, C, device=DEV, generator=gen).permute(0, 3, 1, 2)

    def bn(t):
        C = t.shape[1]
        return F.batch_norm_act(t, torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV),
                                torch.ones(C, device=DEV), True, 0.1, 1e-5, "relu")

    wshape = (Cin, Cout, ks, ks) if transposed else (Cout, Cin, ks, ks)
    w = torch.randn(wshape, device=DEV, generator=gen) * (2.0 / (Cin * ks * ks)) ** 0.5
    b = torch.randn(Cout, device=DEV, generator=gen) * 0.1 if c["bias"] else None
    arena = None
    if c["arena"]:
        w, b = torch.nn.Parameter(w), torch.nn.Parameter(b)
        arena = optim.Adam([w, b], lr=1e-3).arena
        arena.zero_grad(set_to_none=True)
    else:
        w.requires_grad_(True)
        if b is not None:
            b.requires_grad_(True)
    x0 = nhwc(Cin, H, W).requires_grad_(c["image_grad"])
    prev = F.get_conv_precision(), {k: getattr(F, k) for k in c["flags"]}
    F.set_conv_precision(c["mode"])
    for k, v in c["flags"].items():
        setattr(F, k, v)
    raw, grads = [], []
    try:
        with _recording(raw):
            x = bn(x0) if c["feed"] == "bn" else x0
            if x.requires_grad:
                x.retain_grad()
            if c["entry"] == "conv5x5":
                y = F.conv5x5(x, w, b, c["stride"], c["act"])
            elif c["entry"] == "conv2d":
                y = F.conv2d(x, w, b, c["stride"])
            elif c["entry"] == "conv_transpose5x5":
                y = F.conv_transpose5x5(x, w, c["stride"])
            else:
                y = F.conv_transpose2d(x, w, b, c["stride"])
            y.register_hook(grads.append)
            if c["feed"] == "bn":
                bn(y).backward(nhwc(y.shape[1], y.shape[2], y.shape[3]))
            else:
                y.backward(nhwc(y.shape[1], y.shape[2], y.shape[3]))
            torch.cuda.synchronize()
    finally:
        F.set_conv_precision(prev[0])
        for k, v in prev[1].items():
            setattr(F, k, v)
    named = {"x": x, "weight": w, "bias": b, "dy": grads[0], "y": y, "dx": x.grad, "dw": w.grad, "db": None if b is None else b.grad}
    names = {t.data_ptr(): n for n, t in named.items() if t is not None}
    if arena is not None:       # (after the plain names: a gradient that autograd adopted from the arena IS the slice)
        names[arena.grad_view(w).data_ptr()] = "dw@arena"
        names[arena.grad_view(b).data_ptr()] = "db@arena"
    log = []
    for name, args in raw:
        args = [v if kind == "s" else ("null" if v is None else names.get(v, "tmp")) for kind, v in args[:-1]]
        log.append(list(canonical(name, args)))
    dig = {n: _digest(named[n]) for n in ("y", "dx", "dw", "db")} if digests else None
    return log, dig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write {case: log} as JSON")
    ap.add_argument("--digests", action="store_true")
    a = ap.parse_args()
    logs = {}
    for c in CASES:
        logs[c["name"]], dig = run_case(c, a.digests)
        if a.digests:
            print("digest", c["name"], json.dumps(dig, sort_keys=True))
    if a.out:
        with open(a.out, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(l)}" for n, l in logs.items()) + "\n}\n")
    print(f"{len(logs)} cases, {sum(map(len, logs.values()))} launches")


if __name__ == "__main__":
    main()
