"""The loss kernels of csrc/elementwise.hip, each called through the C ABI on NaN-prefilled, sentinel-guarded outputs
(tests/guarded.py) and held to the fp64 references of tests/small_ref.py: tensors to OP_RTOL in rel_err's norm, scalar sums of
positive terms to OP_RTOL of the reference value, vp_sum_f32 to OP_RTOL of sum |x|.  The sizes reach the second (third) trip of every
capped grid-stride loop -- grid_for's 2048 blocks = 524,288 items, reduce_blocks' 1024 blocks = 1,048,576 floats (262,144 for the
L1 partials), 256 blocks for the BE backward -- and the row / group / chunk edges of the single-workgroup kernels.  Every reduction
is run twice and must return the same bits."""
import pytest
import torch

from tests import small_ref as R
from tests.guarded import NAN16, Guards, same_bits
from tests.guarded import api as _api, gen as _gen, scalar_close as _scalar, tensor_close as _tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _probs(n, seed, plant_from=2):
    """p in (0.01, 0.99), t in [0, 1); from n = plant_from on, p in {0, 1} is planted at the first two and the last two elements
    (below that size a single 0 if plant_from is 2: the reductions; nothing otherwise, so that the tiny sizes of the element-wise
    kernels compare ordinary elements and not only the 1e-12 floor)"""
    g = _gen(seed)
    p, t = torch.rand(n, generator=g) * 0.98 + 0.01, torch.rand(n, generator=g)
    if n >= plant_from:
        p[0], p[1], p[-2], p[-1] = 0.0, 1.0, 0.0, 1.0
    elif plant_from == 2:
        p[0] = 0.0
    return p, t


N_REDUCE = [1, 2, 3, 5, 1027, 2 * 1048576 + 4000 + 3]


@pytest.mark.parametrize("n", N_REDUCE)
def test_bce_sum(n):
    _lib, ops, lib = _api()
    p_c, t_c = _probs(n, 100 + n % 97)
    p, t = p_c.to(DEV), t_c.to(DEV)
    ref = R.bce_sum(p_c, t_c)
    runs = []
    for _ in range(2):
        G = Guards()
        out = G.out("out", 1)
        ws, nb = G.ws("ws", lib.vp_reduce_workspace_bytes(n))
        _lib.call("vp_bce_sum_f32", ops._p(p), ops._p(t), n, ops._p(out), ops._p(ws), nb, ops._stream())
        G.check()
        runs.append(out.clone())
    _scalar(runs[0], ref, f"bce_sum n={n}")
    assert same_bits(runs[0], runs[1]), "two runs differ"
    assert same_bits(ops.bce_sum(p, t), runs[0]), "ops.bce_sum differs from the direct call"


@pytest.mark.parametrize("n", N_REDUCE)
def test_vae_loss(n):
    _lib, ops, lib = _api()
    B = 100
    p_c, t_c = _probs(n, 200 + n % 97)
    kl_c = torch.rand(B, generator=_gen(7)) * 40 + 0.5
    p, t, kl = p_c.to(DEV), t_c.to(DEV), kl_c.to(DEV)
    ref = R.vae_loss(p_c, t_c, kl_c, 1.0 / B)
    runs = []
    for _ in range(2):
        G = Guards()
        recon, kl_sum, loss = G.out("recon", 1), G.out("kl_sum", 1), G.out("loss", 1)
        ws, nb = G.ws("ws", lib.vp_reduce_workspace_bytes(n))
        _lib.call("vp_vae_loss_f32", ops._p(p), ops._p(t), n, ops._p(kl), B, ops._p(recon), ops._p(kl_sum), ops._p(loss), 1.0 / B,
                  ops._p(ws), nb, ops._stream())
        G.check()
        runs.append(torch.cat([recon, kl_sum, loss]).clone())
    for i, name in enumerate(("recon", "kl_sum", "loss")):
        _scalar(runs[0][i], ref[i], f"vae_loss {name} n={n}")
    assert same_bits(runs[0], runs[1]), "two runs differ"


@pytest.mark.parametrize("n", N_REDUCE)
def test_sum(n):
    _lib, ops, lib = _api()
    x_c = torch.randn(n, generator=_gen(300 + n % 97))
    x = x_c.to(DEV)
    runs = []
    for _ in range(2):
        G = Guards()
        out = G.out("out", 1)
        ws, nb = G.ws("ws", lib.vp_reduce_workspace_bytes(n))
        _lib.call("vp_sum_f32", ops._p(x), n, ops._p(out), ops._p(ws), nb, ops._stream())
        G.check()
        runs.append(out.clone())
    _scalar(runs[0], R.tensor_sum(x_c), f"sum n={n}", denom=R.abs_sum(x_c))
    assert same_bits(runs[0], runs[1]), "two runs differ"
    assert same_bits(ops.tensor_sum(x), runs[0]), "ops.tensor_sum differs from the direct call"


@pytest.mark.parametrize("n", [1, 3, 6, 2 * 524288 + 77])
def test_bce_bwd(n):
    _lib, ops, lib = _api()
    p_c, t_c = _probs(n, 400 + n % 97, plant_from=5)
    p, t = p_c.to(DEV), t_c.to(DEV)
    gdev = torch.tensor([0.7], device=DEV)
    inner = slice(2, n - 2) if n > 4 else slice(0, 0)      # the elements away from the 1e-12 floor (their scale is 1e12 smaller)
    for gptr, g, gscale in ((None, 1.0, 0.03125), (gdev, 0.7, 1.0 / 3.0)):
        G = Guards()
        dp = G.out("dp", n)
        _lib.call("vp_bce_bwd_f32", ops._p(p), ops._p(t), ops._p(gptr), gscale, ops._p(dp), n, ops._stream())
        G.check()
        ref = R.bce_bwd(p_c, t_c, g, gscale)
        _tensor(dp, ref, f"bce_bwd n={n} g={g}")
        if n > 4:
            _tensor(dp[inner], ref[inner], f"bce_bwd (unclamped elements) n={n} g={g}")
    assert same_bits(ops.bce_bwd(p, t, gdev, 1.0 / 3.0), dp), "ops.bce_bwd differs from the direct call"


@pytest.mark.parametrize("n", [1, 3, 6, 2 * 2097152 + 7])
def test_bce_sigmoid_bwd(n):
    _lib, ops, lib = _api()
    p_c, t_c = _probs(n, 500 + n % 97, plant_from=5)
    p, t = p_c.to(DEV), t_c.to(DEV)
    G = Guards()
    dl = G.out("dlogit", n)
    _lib.call("vp_bce_sigmoid_bwd_f32", ops._p(p), ops._p(t), 0.3, ops._p(dl), n, ops._stream())
    G.check()
    _tensor(dl, R.bce_sigmoid_bwd(p_c, t_c, float(torch.tensor(0.3).item())), f"bce_sigmoid_bwd n={n}")
    assert same_bits(ops.bce_sigmoid_bwd(p, t, 0.3), dl), "ops.bce_sigmoid_bwd differs from the direct call"


@pytest.mark.parametrize("npix,C,Cpad", [(35, 3, 8), (1, 1, 8), (70000, 3, 8)])
def test_bce_sigmoid_bwd_pad_split(npix, C, Cpad):
    """gscale = 0.5 and inputs that are multiples of 2^-24 below 1: gscale * (p - t) is exact in fp32, so the planes can be held bit
    for bit to the split of the (zero-padded) reference tensor"""
    _lib, ops, lib = _api()
    g = _gen(600 + npix % 97)
    p_c, t_c = torch.rand(npix, C, generator=g), torch.rand(npix, C, generator=g)
    p, t = p_c.to(DEV), t_c.to(DEV)
    G = Guards()
    dl = G.out("dlogit", npix, C)
    planes = G.planes("dlogit_split", npix * Cpad)
    _lib.call("vp_bce_sigmoid_bwd_pad_split_f32", ops._p(p), ops._p(t), 0.5, ops._p(dl), ops._pv(planes), npix, C, Cpad, ops._stream())
    G.check()
    assert not (planes == NAN16).any(), "split planes: elements never written"
    ref = R.bce_sigmoid_bwd_pad(p_c, t_c, 0.5, Cpad)
    _tensor(dl, ref[:, :C], f"bce_sigmoid_bwd_pad {(npix, C, Cpad)}")
    assert torch.equal(ref.float().double(), ref)
    want = ops.split_f32(ref.float().to(DEV))
    assert torch.equal(planes, want), "split planes differ from ops.split_f32 of the zero-padded reference"


@pytest.mark.parametrize("n", [1, 255, 257, 600001])
def test_l1_mean(n):
    _lib, ops, lib = _api()
    g = _gen(700 + n % 97)
    a_c, b_c = torch.randn(n, generator=g), torch.randn(n, generator=g)
    b_c[::7] = a_c[::7]
    if n == 1:
        b_c[0] = a_c[0] + 0.75
    a, b = a_c.to(DEV), b_c.to(DEV)
    runs = []
    for _ in range(2):
        G = Guards()
        out = G.out("out", 1)
        ws, nb = G.ws("ws", 2 * lib.vp_reduce_workspace_bytes(n))
        _lib.call("vp_l1_mean_f32", ops._p(a), ops._p(b), n, ops._p(out), ops._p(ws), nb, ops._stream())
        G.check()
        runs.append(out.clone())
    _scalar(runs[0], R.l1_mean(a_c, b_c), f"l1_mean n={n}")
    assert same_bits(runs[0], runs[1]), "two runs differ"
    assert same_bits(ops.l1_mean(a, b), runs[0]), "ops.l1_mean differs from the direct call"
    gdev = torch.tensor([2.5], device=DEV)
    rda, rdb = R.l1_mean_bwd(a_c, b_c, 2.5)
    rda1, _ = R.l1_mean_bwd(a_c, b_c, 1.0)
    for want_a, want_b, gptr, ra in ((True, False, None, rda1), (False, True, None, rda1), (True, True, gdev, rda)):
        G = Guards()
        da = G.out("da", n) if want_a else None
        db = G.out("db", n) if want_b else None
        _lib.call("vp_l1_mean_bwd_f32", ops._p(a), ops._p(b), ops._p(gptr), ops._p(da), ops._p(db), n, ops._stream())
        G.check()
        if want_a:
            _tensor(da, ra, f"l1_mean_bwd da n={n}")
            assert n == 1 or (da[::7] == 0).all(), "da is not exactly 0 where a == b"
        if want_b:
            _tensor(db, -ra, f"l1_mean_bwd db n={n}")
            assert n == 1 or (db[::7] == 0).all(), "db is not exactly 0 where a == b"
    wa, wb = ops.l1_mean_bwd(a, b, gdev, True, True)
    assert same_bits(wa, da) and same_bits(wb, db), "ops.l1_mean_bwd differs from the direct call"


@pytest.mark.parametrize("n", [1, 255, 256, 257, 511, 512, 513, 600, 1100])
def test_half_sqdiff_rowsum(n):
    _lib, ops, lib = _api()
    Rr = 3
    g = _gen(800 + n)
    a_c, b_c = torch.randn(Rr, n, generator=g), torch.randn(Rr, n, generator=g)
    a, b = a_c.to(DEV), b_c.to(DEV)
    runs = []
    for _ in range(2):
        G = Guards()
        out = G.out("out", Rr)
        _lib.call("vp_half_sqdiff_rowsum_f32", ops._p(a), ops._p(b), ops._p(out), Rr, n, ops._stream())
        G.check()
        runs.append(out.clone())
    _scalar(runs[0], R.half_sqdiff_rowsum(a_c, b_c), f"half_sqdiff_rowsum n={n}")
    assert same_bits(runs[0], runs[1]), "two runs differ"
    assert same_bits(ops.half_sqdiff_rowsum(a, b), runs[0]), "ops.half_sqdiff_rowsum differs from the direct call"


@pytest.mark.parametrize("Rr,n", [(7, 11), (3, 349551)])
def test_half_sqdiff_and_bwd(Rr, n):
    _lib, ops, lib = _api()
    g = _gen(900 + Rr)
    a_c, b_c = torch.randn(Rr, n, generator=g), torch.randn(Rr, n, generator=g)
    ge_c, gr_c = torch.randn(Rr, n, generator=g), torch.randn(Rr, generator=g)
    a, b, ge, gr = a_c.to(DEV), b_c.to(DEV), ge_c.to(DEV), gr_c.to(DEV)
    G = Guards()
    out = G.out("out", Rr, n)
    _lib.call("vp_half_sqdiff_f32", ops._p(a), ops._p(b), ops._p(out), Rr * n, ops._stream())
    G.check()
    _tensor(out, R.half_sqdiff(a_c, b_c), f"half_sqdiff {(Rr, n)}")
    assert same_bits(ops.half_sqdiff(a, b), out), "ops.half_sqdiff differs from the direct call"
    for per_row, gt, gt_c in ((0, ge, ge_c), (1, gr, gr_c)):
        rda, rdb = R.half_sqdiff_bwd(a_c, b_c, gt_c, per_row)
        for want_a, want_b in ((True, True), (False, True), (True, False)):
            G = Guards()
            da = G.out("da", Rr, n) if want_a else None
            db = G.out("db", Rr, n) if want_b else None
            _lib.call("vp_half_sqdiff_bwd_f32", ops._p(a), ops._p(b), ops._p(gt), ops._p(da), ops._p(db), Rr, n, per_row, ops._stream())
            G.check()
            if want_a:
                _tensor(da, rda, f"half_sqdiff_bwd da {(Rr, n)} per_row={per_row}")
            if want_b:
                _tensor(db, rdb, f"half_sqdiff_bwd db {(Rr, n)} per_row={per_row}")
    wa, wb = ops.half_sqdiff_bwd(a, b, gr, True, True, False)
    assert wb is None and same_bits(wa, da), "ops.half_sqdiff_bwd differs from the direct call"


@pytest.mark.parametrize("B", [1, 5, 64, 100])
def test_gan_head(B):
    """logits ~ N(0, 3^2); the value that drives each group's log to the 1e-3 floor is planted in every group (-30 among the
    originals, +30 among the reconstructed and the sampled), the opposite one next to it where the group has room"""
    _lib, ops, lib = _api()
    coef = 1.7
    x_c = torch.randn(3 * B, generator=_gen(1000 + B)) * 3
    for grp, floor in ((0, -30.0), (1, 30.0), (2, 30.0)):
        x_c[grp * B] = floor
        if B > 1:
            x_c[grp * B + B - 1] = -floor
    x = x_c.to(DEV)
    rp, rs, rd = R.gan_head(x_c, B, float(torch.tensor(coef).item()))
    first = None
    for has_p, has_s, has_d in ((1, 1, 1), (1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        G = Guards()
        p = G.out("p", 3 * B) if has_p else None
        s = G.out("sums", 3) if has_s else None
        d = G.out("dlogit", 3 * B) if has_d else None
        _lib.call("vp_gan_head_f32", ops._p(x), B, coef, ops._p(p), ops._p(s), ops._p(d), ops._stream())
        G.check()
        tag = f"B={B} outputs={has_p}{has_s}{has_d}"
        if has_p:
            _tensor(p, rp, f"gan_head p {tag}")
        if has_s:
            _scalar(s, rs, f"gan_head sums {tag}")
        if has_d:
            _tensor(d, rd, f"gan_head dlogit {tag}")
        if first is None:
            first = (p.clone(), s.clone(), d.clone())
        elif has_p and has_s and has_d:
            assert all(same_bits(u, v) for u, v in zip(first, (p, s, d))), "two runs differ"


@pytest.mark.parametrize("B,n1,n2", [(4, 3, 2), (1, 1, 0), (37, 5, 3)])
def test_smooth_l1_cat(B, n1, n2):
    """differences straddle |d| = 1; exact +1 and -1 are planted (t = a + 1 with a = 0.5: exact in fp32)"""
    _lib, ops, lib = _api()
    g = _gen(1100 + B)
    a_c = torch.randn(B, n1, generator=g)
    b_c = torch.randn(B, n2, generator=g) if n2 else None
    a_c[0, 0] = 0.5
    if B > 1:
        a_c[1, n1 - 1] = -0.25
    cat = a_c if b_c is None else torch.cat([a_c, b_c], 1)
    t_c = cat + torch.randn(B, n1 + n2, generator=g) * 1.5
    t_c[0, 0] = 1.5
    if B > 1:
        t_c[1, n1 - 1] = -1.25
    assert (t_c[0, 0] - a_c[0, 0]).item() == 1.0
    t, a, b = t_c.to(DEV), a_c.to(DEV), (b_c.to(DEV) if n2 else None)
    scale = 1.0 / B
    rl, rda, rdb = R.smooth_l1_cat(t_c, a_c, b_c, float(torch.tensor(scale).item()))
    first = None
    for has_l, has_g in ((1, 1), (1, 1), (0, 1), (1, 0)):
        G = Guards()
        loss = G.out("loss", 1) if has_l else None
        da = G.out("da", B, n1) if has_g else None
        db = G.out("db", B, n2) if has_g and n2 else None
        _lib.call("vp_smooth_l1_cat_f32", ops._p(t), ops._p(a), ops._p(b), B, n1, n2, scale, ops._p(loss), ops._p(da), ops._p(db),
                  ops._stream())
        G.check()
        tag = f"{(B, n1, n2)} outputs={has_l}{has_g}"
        if has_l:
            _scalar(loss, rl, f"smooth_l1_cat loss {tag}")
        if has_g:
            _tensor(da, rda, f"smooth_l1_cat da {tag}")
            if n2:
                _tensor(db, rdb, f"smooth_l1_cat db {tag}")
        if first is None:
            first = (loss.clone(), da.clone())
        elif has_l and has_g:
            assert same_bits(first[0], loss) and same_bits(first[1], da), "two runs differ"


BE_SHAPES = [(1, 1), (3, 2 * 4096 + 37), (2, 2 * 65536 + 37)]


@pytest.mark.parametrize("B,n", BE_SHAPES)
def test_be_loss(B, n):
    _lib, ops, lib = _api()
    g = _gen(1200 + B)
    x_c = torch.randn(B, n, generator=g) * 3
    t_c = (torch.rand(B, n, generator=g) < 0.4).float()
    x, t = x_c.to(DEV), t_c.to(DEV)
    w, smooth = 0.5, 1.0
    runs = []
    for _ in range(2):
        G = Guards()
        loss, sums = G.out("loss", 1), G.out("sums", B, 4)
        ws, nb = G.ws("ws", lib.vp_be_loss_workspace_bytes(B, n))
        _lib.call("vp_be_loss_fwd_f32", ops._p(x), ops._p(t), ops._p(loss), ops._p(sums), B, n, w, smooth, ops._p(ws), nb, ops._stream())
        G.check()
        runs.append((loss.clone(), sums.clone()))
    (loss, sums) = runs[0]
    assert same_bits(loss, runs[1][0]) and same_bits(sums, runs[1][1]), "two runs differ"
    rl, rs, _ = R.be_loss(x_c, t_c, w, smooth)
    _scalar(loss, rl, f"be_loss loss {(B, n)}")
    _scalar(sums, rs, f"be_loss sums {(B, n)}")
    wl, wsums = ops.be_loss_fwd(x, t, w, smooth)
    assert same_bits(wl, loss) and same_bits(wsums, sums), "ops.be_loss_fwd differs from the direct call"
    gdev = torch.tensor([1.3], device=DEV)
    for gptr, gv in ((None, 1.0), (gdev, float(gdev.item()))):
        G = Guards()
        dx = G.out("dx", B, n)
        _lib.call("vp_be_loss_bwd_f32", ops._p(x), ops._p(t), ops._p(sums), ops._p(gptr), ops._p(dx), B, n, w, smooth, ops._stream())
        G.check()
        _tensor(dx, R.be_loss(x_c, t_c, w, smooth, gv)[2], f"be_loss dx {(B, n)} g={gv:.1f}")
    assert same_bits(ops.be_loss_bwd(x, t, sums, gdev, w, smooth), dx), "ops.be_loss_bwd differs from the direct call"


@pytest.mark.parametrize("B,n", BE_SHAPES)
def test_dice_loss(B, n):
    _lib, ops, lib = _api()
    g = _gen(1300 + B)
    p_c = torch.rand(B, n, generator=g) * 0.98 + 0.01
    t_c = (torch.rand(B, n, generator=g) < 0.4).float()
    p, t = p_c.to(DEV), t_c.to(DEV)
    smooth = 1.0
    runs = []
    for _ in range(2):
        G = Guards()
        loss, sums = G.out("loss", 1), G.out("sums", B, 4)
        ws, nb = G.ws("ws", lib.vp_be_loss_workspace_bytes(B, n))
        _lib.call("vp_dice_loss_fwd_f32", ops._p(p), ops._p(t), ops._p(loss), ops._p(sums), B, n, smooth, ops._p(ws), nb, ops._stream())
        G.check()
        runs.append((loss.clone(), sums.clone()))
    (loss, sums) = runs[0]
    assert same_bits(loss, runs[1][0]) and same_bits(sums, runs[1][1]), "two runs differ"
    rl, rs, _ = R.dice_loss(p_c, t_c, smooth)
    _scalar(loss, rl, f"dice_loss loss {(B, n)}")
    _scalar(sums, rs, f"dice_loss sums {(B, n)}")
    wl, wsums = ops.dice_loss_fwd(p, t, smooth)
    assert same_bits(wl, loss) and same_bits(wsums, sums), "ops.dice_loss_fwd differs from the direct call"
    gdev = torch.tensor([0.6], device=DEV)
    for gptr, gv in ((None, 1.0), (gdev, float(gdev.item()))):
        G = Guards()
        dp = G.out("dp", B, n)
        _lib.call("vp_dice_loss_bwd_f32", ops._p(p), ops._p(t), ops._p(sums), ops._p(gptr), ops._p(dp), B, n, smooth, ops._stream())
        G.check()
        _tensor(dp, R.dice_loss(p_c, t_c, smooth, gv)[2], f"dice_loss dp {(B, n)} g={gv:.1f}")
    assert same_bits(ops.dice_loss_bwd(p, t, sums, gdev, smooth), dp), "ops.dice_loss_bwd differs from the direct call"


@pytest.mark.parametrize("B,Z", [(1, 1), (3, 64), (5, 100), (2, 300000)])
def test_latent(B, Z):
    _lib, ops, lib = _api()
    g = _gen(1400 + B)
    mu_c, eps_c = torch.randn(B, Z, generator=g), torch.randn(B, Z, generator=g)
    lv_c = torch.rand(B, Z, generator=g) * 10 - 6
    dz_c, gkl_c = torch.randn(B, Z, generator=g), torch.randn(B, generator=g)
    mu, eps, lv, dz, gkl = (v.to(DEV) for v in (mu_c, eps_c, lv_c, dz_c, gkl_c))
    rz, rkl = R.latent_fwd(mu_c, lv_c, eps_c)
    keep = None
    for has_kl in (True, True, False):
        G = Guards()
        z = G.out("z", B, Z)
        kl = G.out("kl", B) if has_kl else None
        _lib.call("vp_latent_fwd_f32", ops._p(mu), ops._p(lv), ops._p(eps), ops._p(z), ops._p(kl), B, Z, ops._stream())
        G.check()
        _tensor(z, rz, f"latent z {(B, Z)} kl={has_kl}")
        if has_kl:
            _tensor(kl, rkl, f"latent kl {(B, Z)}")
            keep = keep or (z.clone(), kl.clone())
            assert same_bits(keep[0], z) and same_bits(keep[1], kl), "two runs differ"
    wz, wkl = ops.latent_fwd(mu, lv, eps)
    assert same_bits(wz, keep[0]) and same_bits(wkl, keep[1]), "ops.latent_fwd differs from the direct call"
    sc = 0.25
    for use_dz, use_gkl, scalar in ((1, 0, 0.0), (0, 1, 0.0), (0, 0, sc), (1, 1, sc)):
        G = Guards()
        dmu, dlv = G.out("dmu", B, Z), G.out("dlogvar", B, Z)
        _lib.call("vp_latent_bwd_f32", ops._p(mu), ops._p(lv), ops._p(eps), ops._p(dz if use_dz else None),
                  ops._p(gkl if use_gkl else None), scalar, ops._p(dmu), ops._p(dlv), B, Z, ops._stream())
        G.check()
        rdmu, rdlv = R.latent_bwd(mu_c, lv_c, eps_c, dz_c if use_dz else None, gkl_c if use_gkl else None, scalar)
        tag = f"{(B, Z)} dz={use_dz} gkl={use_gkl} scalar={scalar}"
        _tensor(dmu, rdmu, f"latent dmu {tag}")
        _tensor(dlv, rdlv, f"latent dlogvar {tag}")
    wdmu, wdlv = ops.latent_bwd(mu, lv, eps, dz, gkl, sc)
    assert same_bits(wdmu, dmu) and same_bits(wdlv, dlv), "ops.latent_bwd differs from the direct call"
