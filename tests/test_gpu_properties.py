"""Size-independent properties at BASELINE.json's FULL sizes (128 x 128 x 3, latent 128, 32 images per GPU), where the CPU oracle
is too slow to be the checker for every layer: the three convolution families must be each other's adjoints and bilinear, and
BatchNorm's outputs / input gradients must satisfy the identities of the normalisation.  Computed entirely on the device through
the C ABI; the reference values are fp64 sums of the same device results -- and, for sampled outputs of every family, fp64 direct
sums of the convolution's definition (tests/conv_ref.py)."""
import pytest
import torch

from tests import conv_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (name, Cbig, Csmall, Hs): the 5x5 stride-2 layers on the split-bf16 / exact-f32 kernels (big = the 2x larger image side)
def _layers(img, L):
    size = 64 << (L - 1)
    out = [(f"enc{i}", 64 << (i - 1), 64 << i, img >> (i + 1)) for i in range(1, L)]
    for i in range(L):
        cin, cout = (size if i == 0 else size >> (i - 1)), size >> i
        out.append((f"dec{i}", cout, cin, 8 << i))
    return out


# BASELINE.json configs at their per-GPU launch shapes: every tile / split-K branch choose_tile16, wgrad_nsplit, the split-K
# rules of conv16.hip and (where enabled) the pipelined-kernel dispatch take on them runs under test
CONFIGS = {"c3_128px_b32": (32, _layers(128, 4)),           # config 3 (and 4): the benchmark shard
           "c2_64px_b128": (128, _layers(64, 3)),           # config 2
           "c5_256px_b8": (8, _layers(256, 5)),             # config 5: 256 x 256, iter_level 5, 64 images over 8 GPUs
           "c3_128px_b128": (128, _layers(128, 4))}         # batch sweep of bench.py
CASES = [(cfg, *ly) for cfg, (_, lys) in CONFIGS.items() for ly in lys]
B = 32


def _dot(a, b):
    return (a.double() * b.double()).sum().item()


@pytest.mark.parametrize("cfg,name,Cb,Cs,Hs", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_conv_families_are_adjoint_and_bilinear_at_full_size(cfg, name, Cb, Cs, Hs, precision):
    from vae_play_amd import ops
    B = CONFIGS[cfg][0]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Hb = 2 * Hs
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)
    x, x2 = cl(torch.randn(B, Cb, Hb, Hb, generator=g)), cl(torch.randn(B, Cb, Hb, Hb, generator=g))
    y = cl(torch.randn(B, Cs, Hs, Hs, generator=g))
    w = (torch.randn(Cs, Cb, 5, 5, generator=g) * 0.05).to(DEV)
    if precision == "bf16x3":
        p0, p1 = ops.pack_w5_split(w, True, True)
        gather = lambda t: ops.conv5_gather_bf16x3(ops.split_f32(t), t.shape, p0, Cs, None, 2, 0)
        scatter = lambda t: ops.conv5_scatter_bf16x3(ops.split_f32(t), t.shape, p1, Cb, 2)
        wgrad = lambda big, small: ops.conv5_wgrad_bf16x3(ops.split_f32(big), tuple(big.shape), ops.split_f32(small), tuple(small.shape), 2)
        tol = 3e-5
    else:
        p0, p1 = ops.pack_w5(w, True, True)
        gather = lambda t: ops.conv5_gather(t, p0, None, 2, 0)
        scatter = lambda t: ops.conv5_scatter(t, p1, 2)
        wgrad = lambda big, small: ops.conv5_wgrad(big, small, 2)
        tol = 3e-6
    cx = gather(x)
    # <conv(x), y> = <x, conv^T(y)> = <w, wgrad(x, y)>: gather, scatter and weight-gradient kernels are one bilinear form
    lhs = _dot(cx, y)
    scale = (cx.double().pow(2).sum().sqrt() * y.double().pow(2).sum().sqrt()).item()
    assert abs(lhs - _dot(x, scatter(y))) <= tol * scale, f"{name}: scatter is not the adjoint of gather"
    assert abs(lhs - _dot(w, wgrad(x, y))) <= tol * scale, f"{name}: the weight gradient is not the form's derivative"
    # linearity in the activation
    a, b = 0.75, -1.5
    mix = gather(a * x + b * x2)
    ref = a * cx + b * gather(x2)
    err = ((mix - ref).double().pow(2).sum().sqrt() / ref.double().pow(2).sum().sqrt()).item()
    assert err <= tol * 4, f"{name}: gather not linear ({err:.2e})"
    _check_epilogue_statistics(name, x, p0, p1, y, Cb, Cs, Hs, B, cx, precision)


def _check_epilogue_statistics(name, x, p0, p1, y, Cb, Cs, Hs, B, cx, precision="bf16x3"):
    """vp_conv5_*_stats_{bf16x3,f32,f16}: same convolution output as the plain entry point, and mean / rstd / running statistics equal
    to the stand-alone statistics kernels' (which read the activation again) -- for every launch shape that can emit them.  p0 / p1 /
    cx: the packed weights and the plain gather output of `precision` (f16x2: fp16-pair planes, three products as the forward layers
    run them)."""
    from vae_play_amd import _lib, ops
    lib = _lib.load()
    if precision == "f32":
        query, suffix, extra = lib.vp_conv5_stats_f32_workspace_bytes, "f32", ()
        prep, ptr = (lambda t: t), ops._p
        plain_scatter = lambda: ops.conv5_scatter(y, p1, 2)
    elif precision == "f16x2":
        query, suffix, extra = lib.vp_conv5_stats_f16_workspace_bytes, "f16", (3,)
        prep, ptr = (lambda t: ops.split_f32(t, ops.SPLIT_F16)), ops._pv
        plain_scatter = lambda: ops.conv5_scatter_f16(prep(y), y.shape, p1, Cb, 2, products=3)
    else:
        query, suffix, extra = lib.vp_conv5_stats_workspace_bytes, "bf16x3", ()
        prep, ptr = ops.split_f32, ops._pv
        plain_scatter = lambda: ops.conv5_scatter_bf16x3(ops.split_f32(y), y.shape, p1, Cb, 2)
    for family in (0, 1):
        nbytes = query(family, B, Hs, Hs, Cb, Cs, 2)
        if not nbytes:
            continue
        ws = torch.empty(nbytes // 4, device=DEV)
        if family == 0:
            ref_out, Cn, R = cx, Cs, B * Hs * Hs
            out = torch.empty_like(ref_out)
            inp, wq, name_ = prep(x), p0, f"vp_conv5_gather_stats_{suffix}"
            geom = (B, Hs, Hs, Cb, Cs, 2)
        else:
            ref_out, Cn, R = plain_scatter(), Cb, B * 4 * Hs * Hs
            out = torch.empty_like(ref_out)
            inp, wq, name_ = prep(y), p1, f"vp_conv5_scatter_stats_{suffix}"
            geom = (B, Hs, Hs, Cs, Cb, 2)
        mean, rstd = torch.empty(Cn, device=DEV), torch.empty(Cn, device=DEV)
        rm, rv = torch.zeros(Cn, device=DEV), torch.ones(Cn, device=DEV)
        _lib.call(name_, ptr(inp), ptr(wq), ops._p(out), *geom, *extra, 1e-5, 0.9, ops._p(mean), ops._p(rstd), ops._p(rm), ops._p(rv),
                  ops._p(ws), nbytes, ops._stream())
        # The epilogue changes no arithmetic of the kernel it runs in.  f32 (conv32.hip) and f16x2 (conv16_f16.hip): the statistics
        # launch runs the very kernel of the plain launch -- conv_gather / conv_scatter (csrc/conv_exec.h) on the
        # same problem type, tile and split rule, the statistics pointer is a kernel argument -- so the outputs must be equal bit for bit.
        # bf16x3, round 3: a plain launch may take ANOTHER kernel than the statistics launch of the same shape -- the pipelined kernel
        # on the v_mfma_f32_16x16x32_bf16 form (launch_plan.h plan_conv: the gather shapes with 256 output columns and 16 K - 64 K rows),
        # whose accumulator layout the epilogue does not read -- and that form equals the 32x32x16 kernels to rounding, not bit for
        # bit: the outputs must then agree to 2e-6 of their RMS.
        if precision != "bf16x3":
            assert torch.equal(out, ref_out), f"{name} {precision} family {family}: the statistics launch changed the convolution's output"
        elif not torch.equal(out, ref_out):
            rms = ref_out.double().pow(2).mean().sqrt().item()
            dmax = (out.double() - ref_out.double()).abs().max().item()
            assert dmax <= 2e-6 * max(rms, 1e-30) * 16, f"{name} family {family}: the statistics launch differs from the plain one by {dmax:.2e} (rms {rms:.2e})"
        rm2, rv2 = torch.zeros(Cn, device=DEV), torch.ones(Cn, device=DEV)
        mean2, rstd2 = ops.bn_stats(out, 1e-5, 0.9, rm2, rv2)
        xd = out.double()
        m64 = xd.mean(dim=(0, 2, 3)); v64 = xd.var(dim=(0, 2, 3), unbiased=False)
        sig = v64.sqrt()
        assert ((mean.double() - m64).abs() / sig).max().item() <= 1e-5, f"{name} family {family}: mean"
        assert ((rstd.double() - (v64 + 1e-5).rsqrt()).abs() * sig).max().item() <= 1e-5, f"{name} family {family}: rstd"
        assert ((mean - mean2).abs() / sig.float()).max().item() <= 1e-5 and ((rstd - rstd2).abs() * sig.float()).max().item() <= 1e-5
        assert ((rm - rm2).abs() / sig.float()).max().item() <= 1e-5 and ((rv - rv2).abs() / v64.float()).max().item() <= 1e-5, "running buffers"


# Direct-sum tolerances, fixed from the arithmetic before any measurement.  A sample is r = sum_i a_i b_i over K terms and
# A = sum |a_i b_i|; K >= 392 at every sampled element here (a border gather output: 3 x 3 taps x Cb >= 64; a border scatter output:
# 2 x 2 taps x Cs >= 128; a border tap of the weight gradient at config 5's 8 x 8 layers: 8 images x 7 x 7 pixels).  Random rounding
# gives |out - r| / A ~ u * O(1) for the fp32 accumulation (u = 2^-24 = 6e-8) plus d * 1.57 / sqrt(K) for a relative operand error of
# rms d per term (for Gaussian operands sqrt(sum (a_i b_i)^2) / A = 1.57 / sqrt(K), at most 1.57 / sqrt(392) = 0.079):
#   f32      exact products                                         1.6 u                         = 1.0e-7  ->  tau 1e-6
#   bf16x3   hi + lo keep 16 bits per operand (d <= 2^-17 each;     1.6 u + 2 * 2^-17 * 0.079     = 1.3e-6  ->  tau 1e-5
#            the dropped lo * lo product is below 2^-18)
#   f16x2/3  hi + lo keep 22 bits per operand (d <= 2^-20 each,     1.6 u + 2 * 2^-20 * 0.079     = 2.5e-7  ->  tau 1e-5
#            allowing for the partly subnormal lo plane of a 0.05-scale weight)
#   f16x2/2  one operand keeps its fp16 hi plane only: 11          2.1e-4 * 0.079                = 1.7e-5  ->  tau 1e-4
#            significant bits, d = 2.1e-4 rms
# Every tau is at least 6x its estimate; a failure is a finding to explain, never a reason to raise tau.
# Finding: the far border of the scatter breaks the K >= 392 premise -- big row Hb - 1 is reached by tap r = 3 alone, so
# the corner (Hb - 1, Wb - 1) sums Cs terms only (128 at dec3), where the two-product estimate is 2.1e-4 * 1.57 / sqrt(128) = 2.9e-5
# and the measured 1.0e-4 - 1.1e-4 is the expected ~4 sigma of ~12 K samples, not a kernel error.  So the two-product forms are held
# to tau 1e-4 against the operation where a sample has >= 392 terms, and, at EVERY sample, to the three-product tau 1e-5 against the
# arithmetic they declare: the operand that keeps its hi plane only rounded to fp16 (round to nearest, as the split producers do).
MIN_TERMS = 392
TAU = {"f32": 1e-6, "bf16x3": 1e-5, "f16x2/3": 1e-5, "f16x2/2": 1e-4, "f16x2/2 declared": 1e-5}
GSCALE = 16.0     # power-of-two scale of the operand in the gradient position of the two-product launches (undone by out_scale)


def _where(family, i, pts, ncol, cs=None, cb=None):
    if family == "wgrad":
        a, rest = divmod(i, len(cb) * 25)
        c, tap = divmod(rest, 25)
        return f"dW[cs={cs[a]}][cb={cb[c]}] tap (r={tap // 5}, q={tap % 5})"
    j, ch = divmod(i, ncol)
    return f"image {pts[j][0]}, pixel ({pts[j][1]}, {pts[j][2]}), channel {ch}"


@pytest.mark.parametrize("cfg,name,Cb,Cs,Hs", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f16x2"])
def test_conv_families_match_the_direct_sum_at_full_size(cfg, name, Cb, Cs, Hs, precision):
    """Sampled outputs of gather, scatter and weight gradient against fp64 sums of the convolution's definition (tests/conv_ref.py):
    |out - r| <= tau * A on every sample -- at the borders, in every stride-2 phase, at the edges of the channel tiles and on all
    25 taps, where a consistent permutation (transposed taps, a mirrored phase map, a channel order) escapes the bilinear-form test."""
    from vae_play_amd import ops
    B = CONFIGS[cfg][0]
    Hb = 2 * Hs
    seed = sum(map(ord, cfg + name))
    gen = torch.Generator(device=DEV).manual_seed(seed)
    # NHWC storage, logical NCHW: generated on the device (a 0.5 GB activation never visits the host)
    x = torch.randn(B, Hb, Hb, Cb, device=DEV, generator=gen).permute(0, 3, 1, 2)
    y = torch.randn(B, Hs, Hs, Cs, device=DEV, generator=gen).permute(0, 3, 1, 2)
    w = torch.randn(Cs, Cb, 5, 5, device=DEV, generator=gen) * 0.05
    gp, sp = conv_ref.gather_points(B, Hs, seed), conv_ref.scatter_points(B, Hb, seed)
    cs, cb = conv_ref.edge_channels(Cs), conv_ref.edge_channels(Cb)
    rg, Ag = conv_ref.gather_ref(x, w, gp)
    rs, As = conv_ref.scatter_ref(y, w, sp)
    rw, Aw = conv_ref.wgrad_ref(x, y, cs, cb)

    outs = []      # (family, tau key, gathered samples, r, A, sample list, channels)
    if precision == "f32":
        p0, p1 = ops.pack_w5(w, True, True)
        cx = ops.conv5_gather(x, p0, None, 2)
        outs += [("gather", "f32", conv_ref.take(cx, gp), rg, Ag, gp, Cs),
                 ("scatter", "f32", conv_ref.take(ops.conv5_scatter(y, p1, 2), sp), rs, As, sp, Cb),
                 ("wgrad", "f32", ops.conv5_wgrad(x, y, 2)[cs][:, cb], rw, Aw, None, None)]
    elif precision == "bf16x3":
        p0, p1 = ops.pack_w5_split(w, True, True)
        xs, ys = ops.split_f32(x), ops.split_f32(y)
        outs += [("gather", "bf16x3", conv_ref.take(ops.conv5_gather_bf16x3(xs, x.shape, p0, Cs, None, 2), gp), rg, Ag, gp, Cs),
                 ("scatter", "bf16x3", conv_ref.take(ops.conv5_scatter_bf16x3(ys, y.shape, p1, Cb, 2), sp), rs, As, sp, Cb),
                 ("wgrad", "bf16x3", ops.conv5_wgrad_bf16x3(xs, tuple(x.shape), ys, tuple(y.shape), 2)[cs][:, cb], rw, Aw, None, None)]
    else:
        F16 = ops.SPLIT_F16
        p0, p1 = ops.pack_w5_split(w, True, True, fmt=F16)
        xs, ys = ops.split_f32(x, F16), ops.split_f32(y, F16)
        xg, yg = ops.split_f32(x, F16, GSCALE), ops.split_f32(y, F16, GSCALE)
        cx = ops.conv5_gather_f16(xs, x.shape, p0, Cs, None, 2, products=3)
        g2 = conv_ref.take(ops.conv5_gather_f16(xg, x.shape, p0, Cs, None, 2, products=2, out_scale=1 / GSCALE), gp)
        s2 = conv_ref.take(ops.conv5_scatter_f16(yg, y.shape, p1, Cb, 2, products=2, out_scale=1 / GSCALE), sp)
        w2 = ops.conv5_wgrad_f16x2(xs, tuple(x.shape), yg, tuple(y.shape), 2, out_scale=1 / GSCALE)[cs][:, cb]
        many = (conv_ref.scatter_terms(sp, Hs, Hs, Cs) >= MIN_TERMS).to(DEV)       # gather and wgrad samples all have >= 392 terms
        wh = w.half().float()                                                       # the hi-only operands of the two-product forms
        outs += [("gather", "f16x2/3", conv_ref.take(cx, gp), rg, Ag, gp, Cs),
                 ("gather", "f16x2/2", g2, rg, Ag, gp, Cs),
                 ("gather", "f16x2/2 declared", g2, *conv_ref.gather_ref(x, wh, gp), gp, Cs),
                 ("scatter", "f16x2/3", conv_ref.take(ops.conv5_scatter_f16(ys, y.shape, p1, Cb, 2, products=3), sp), rs, As, sp, Cb),
                 ("scatter", "f16x2/2", s2, rs, torch.where(many[:, None], As, torch.inf), sp, Cb),
                 ("scatter", "f16x2/2 declared", s2, *conv_ref.scatter_ref(y, wh, sp), sp, Cb),
                 ("wgrad", "f16x2/2", w2, rw, Aw, None, None),
                 ("wgrad", "f16x2/2 declared", w2, *conv_ref.wgrad_ref(x.half().float(), y, cs, cb), None, None)]
    report = []
    for family, key, got, r, A, pts, ncol in outs:
        err, i = conv_ref.worst(got, r, A)
        report.append(f"{family}[{key}] {err:.2e}")
        assert err <= TAU[key], (f"{cfg} {name} {precision} {family}: |out - r| = {err:.2e} * A > tau {TAU[key]:.0e} at "
                                 + _where(family, i, pts, ncol, cs, cb))
    print(f"direct-sum err/A {cfg} {name} {precision}: " + ", ".join(report))
    if precision == "f16x2":      # the other modes' statistics launches run in the adjointness test
        _check_epilogue_statistics(name, x, p0, p1, y, Cb, Cs, Hs, B, cx, precision)


@pytest.mark.parametrize("C,H", [(64, 64), (64, 128), (512, 8)])
def test_batchnorm_identities_at_full_size(C, H):
    from vae_play_amd import functional as FH
    B = 32
    g = torch.Generator().manual_seed(C + H)
    x = (torch.randn(B, C, H, H, generator=g) * 1.7 + torch.randn(1, C, 1, 1, generator=g) * 3).to(DEV)
    x = x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV).requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.3).to(DEV).requires_grad_(True)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y = FH.batch_norm_act(x, gamma, beta, rm, rv, True, 0.9, 1e-5, None, 0.0)
    yd = y.detach().double()
    m = yd.mean(dim=(0, 2, 3)); v = yd.var(dim=(0, 2, 3), unbiased=False)
    assert (m - beta.detach().double()).abs().max().item() <= 2e-5, "mean of the normalised output must be beta"
    assert ((v.sqrt() - gamma.detach().double()).abs() / gamma.detach().double()).max().item() <= 2e-5, "std must be gamma"
    gy = torch.randn(y.shape, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    y.backward(gy)
    dx = x.grad.double()
    xhat = ((x.detach().double() - x.detach().double().mean(dim=(0, 2, 3), keepdim=True))
            / x.detach().double().var(dim=(0, 2, 3), unbiased=False, keepdim=True).add(1e-5).sqrt())
    n = dx.abs().sum(dim=(0, 2, 3))
    # the input gradient of a batch-normalised layer is orthogonal to 1 and to xhat, channel by channel
    assert (dx.sum(dim=(0, 2, 3)).abs() / n).max().item() <= 1e-5
    assert ((dx * xhat).sum(dim=(0, 2, 3)).abs() / n).max().item() <= 1e-5
    assert ((beta.grad.double() - gy.double().sum(dim=(0, 2, 3))).abs() / gy.double().abs().sum(dim=(0, 2, 3))).max().item() <= 1e-5
