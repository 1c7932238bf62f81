"""Two builds of libvaeplay_hip.so, one process: every entry point of csrc/bn.hip over the case list of tests/norm_cases.py, on
guarded buffers (NaN-prefilled, 64 sentinels each side, exact-size workspaces), and every output compared bit for bit: y, dx, the split
planes, mean, rstd, the running statistics, dgamma, dbeta, the saturation flag and the workspace queries.
usage: python tools/ab_norm_bits.py --ref-lib <the other build's libvaeplay_hip.so> [--lib <this build's>]
Exit status 0 when nothing differs."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import norm_cases as N  # noqa: E402
from tests.guarded import Guards  # noqa: E402

BIG_SCALE = 2.0 ** 20        # |dx| ~ 1 times this leaves fp16's range: the saturation flag is set


def bn_case(L, R, C, act, full):
    """every BatchNorm entry point at one shape and activation -> {name: tensor}.  full: gamma, beta and running statistics given,
    batch_stats = 1; else all of them null and batch_stats = 0."""
    G, out = Guards(), {}
    x, dy, gamma, beta, _ = N.inputs(1, R, C, seed=act)
    x, dy = x[0], dy[0]
    if not full:
        gamma = beta = None
    bs = 1 if full else 0
    out["ws_bytes"] = torch.tensor([L.h.vp_bn_workspace_bytes(R, C)])
    mean, rstd, rm, rv = N.bn_stats(L, G, x, R, C, running=full)
    out.update(mean=mean, rstd=rstd, running_mean=rm, running_var=rv)
    kinds = [("plain", 0, 1.0)]
    if C % 4 == 0:
        kinds += [("split", 0, 1.0), ("planes", 0, 1.0), ("fmt", 0, 1.0), ("fmt", 1, 1.0)]
    for kind, fmt, _ in kinds:
        y, ys = N.bn_fwd(L, G, kind, x, mean, rstd, gamma, beta, R, C, act, fmt)
        out[f"fwd {kind}{fmt} y"], out[f"fwd {kind}{fmt} planes"] = y, ys
    if C % 4 == 0:
        kinds += [("fmt", 1, 4096.0), ("sat", 0, 1.0), ("sat", 1, 4096.0), ("sat", 1, BIG_SCALE)]
    for kind, fmt, scale in kinds:
        res = N.bn_bwd(L, G, kind, x, dy, mean, rstd, gamma, beta, R, C, act, bs, full, fmt, scale)
        for t, what in zip(res, ("dx", "planes", "dgamma", "dbeta", "saturated")):
            out[f"bwd {kind}{fmt}x{scale:g} {what}"] = t
    if R <= 64 and C % 4 == 0:
        y, m, r, rm, rv = N.bn_small_fwd(L, G, x, gamma, beta, R, C, act, running=full)
        out.update({"small y": y, "small mean": m, "small rstd": r, "small running_mean": rm, "small running_var": rv})
        for t, what in zip(N.bn_small_bwd(L, G, x, dy, m, r, gamma, beta, R, C, act, bs), ("dx", "dgamma", "dbeta")):
            out[f"small {what}"] = t
    out["act y"], out["act dx"] = N.act_fwd_bwd(L, G, x, dy, act)
    G.check()
    return out


def batched_case(L, B, R, C, act):
    """InstanceNorm and the pair blend (norm 0 and 1) at one shape and activation -> {name: tensor}"""
    G, out = Guards(), {}
    x, dy = N.inputs(B, R, C, seed=act)[:2]
    out["ws_bytes"] = torch.tensor([L.h.vp_instnorm_workspace_bytes(B, R, C), L.h.vp_pair_blend_workspace_bytes(B, R, C)])
    for split in ((False, True) if C % 4 == 0 else (False,)):
        y, mean, rstd, ys = N.inorm_fwd(L, G, x, B, R, C, act, split)
        dx, ds = N.inorm_bwd(L, G, x, dy, mean, rstd, B, R, C, act, split)
        for t, what in ((y, "y"), (mean, "mean"), (rstd, "rstd"), (ys, "y planes"), (dx, "dx"), (ds, "dx planes")):
            out[f"instnorm split={split} {what}"] = t
        u, _, _, _, label = N.inputs(B, R, 2 * C, seed=act)
        for norm in (0, 1):         # (act = none with norm = 0: the backward does not read u)
            y, mean, rstd, ys = N.pair_fwd(L, G, u, label, B, R, C, norm, act, split)
            du, ds = N.pair_bwd(L, G, u, dy, label, mean, rstd, B, R, C, norm, act, split)
            for t, what in ((y, "y"), (mean, "mean"), (rstd, "rstd"), (ys, "y planes"), (du, "du"), (ds, "du planes")):
                out[f"pair norm={norm} split={split} {what}"] = t
    G.check()
    return out


def differences(a, b):
    assert a.keys() == b.keys()
    bad = []
    for k in a:
        if (a[k] is None) != (b[k] is None):
            bad.append(k)
        elif a[k] is not None:
            ta, tb = a[k].detach().cpu().contiguous(), b[k].detach().cpu().contiguous()
            if ta.dtype == torch.float32:
                ta, tb = ta.view(torch.int32), tb.view(torch.int32)
            if ta.shape != tb.shape or not torch.equal(ta, tb):
                bad.append(k)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-lib", required=True)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    from vae_play_amd import _lib
    new, ref = N.Lib(os.path.abspath(a.lib or _lib.LIB_PATH)), N.Lib(os.path.abspath(a.ref_lib))
    cases = [(bn_case, (R, C, act, full)) for R, C in N.BN_SHAPES for act in N.ACTS for full in (True, False)]
    cases += [(batched_case, (B, R, C, act)) for B, R, C in N.BATCHED for act in N.ACTS]
    outputs = failures = saturated = 0
    for fn, args in cases:
        got, want = fn(new, *args), fn(ref, *args)
        bad = differences(got, want)
        outputs += sum(t is not None for t in got.values())
        saturated += sum(int(t.item()) for k, t in got.items() if k.endswith("saturated") and t is not None)
        if bad:
            failures += 1
            print(f"DIFFERENT {fn.__name__}{args}: {bad}")
    print(f"ab_norm_bits: {len(cases)} cases, {outputs} outputs compared, {saturated} set the saturation flag, {failures} cases differ")
    return 1 if failures or not saturated else 0


if __name__ == "__main__":
    sys.exit(main())
