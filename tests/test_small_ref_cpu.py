"""tests/small_ref.py against torch's own float64 operators and autograd (no GPU): both sides are float64, so they may differ by
rounding only -- 1e-12 in tests.util.rel_err's norm.  The shapes are the small edge shapes of the GPU tests."""
import pytest
import torch
import torch.nn.functional as F

from tests import small_ref as R
from tests.util import rel_err

TOL = 1e-12


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, what):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    e = rel_err(a.reshape(b.shape), b)
    assert e <= TOL, f"{what}: rel err {e:.3e}"


@pytest.mark.parametrize("B,C,H,W", [(1, 1, 1, 1), (2, 3, 5, 7), (1, 33, 1, 65), (2, 31, 3, 11)])
def test_layout(B, C, H, W):
    x = torch.randn(B, C, H, W, generator=_g(1))
    nhwc = R.nchw_to_nhwc(x)
    assert nhwc.shape == (B, H, W, C) and nhwc.is_contiguous()
    assert torch.equal(nhwc, x.double().contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1))
    assert torch.equal(R.nhwc_to_nchw(nhwc), x.double())
    for b, c, h, w in ((0, 0, 0, 0), (B - 1, C - 1, H - 1, W - 1), (B - 1, C // 2, H // 2, W - 1)):
        assert nhwc[b, h, w, c].item() == x[b, c, h, w].item()
    for Cout in {C, max(1, C - 2), 1}:
        assert torch.equal(R.slice_channels(nhwc, Cout), x.double()[:, :Cout].permute(0, 2, 3, 1))


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 1), (2, 3, 5, 4)])
def test_add_coords(B, H, W, C, normalize):
    """the module's forward (models/blocks.py: AddCoords) restated on NCHW with torch ops"""
    x = torch.randn(B, H, W, C, generator=_g(2)).double()
    xn = x.permute(0, 3, 1, 2)
    ci = torch.arange(0, W, dtype=torch.float64).reshape(1, 1, 1, -1).repeat(B, 1, H, 1)
    cj = torch.arange(0, H, dtype=torch.float64).reshape(1, 1, -1, 1).repeat(B, 1, 1, W)
    if normalize:
        ci, cj = (ci / W - 0.5) / 0.5, (cj / H - 0.5) / 0.5
    want = torch.cat([xn, ci, cj], dim=1).permute(0, 2, 3, 1)
    got = R.add_coords(x, normalize)
    assert torch.equal(got[..., :C], x)
    _close(got, want, "add_coords")


@pytest.mark.parametrize("kind", [R.ACT_RELU, R.ACT_LRELU, R.ACT_TANH, R.ACT_SIGMOID])
def test_activations(kind):
    x = (torch.randn(300, generator=_g(3)) * 3).double()
    x[:4] = torch.tensor([0.0, -0.0, 20.0, -20.0], dtype=torch.float64)
    slope = 0.02
    fn = {R.ACT_RELU: torch.relu, R.ACT_LRELU: lambda v: F.leaky_relu(v, slope), R.ACT_TANH: torch.tanh,
          R.ACT_SIGMOID: torch.sigmoid}[kind]
    xr = x.clone().requires_grad_(True)
    y = fn(xr)
    dy = torch.randn(300, generator=_g(4)).double()
    y.backward(dy)
    _close(R.act(x, kind, slope), y.detach(), "act")
    want = xr.grad.clone()
    if kind == R.ACT_LRELU:
        want[:2] = dy[:2] * slope      # at x == 0 the kernels' rule is y > 0 ? 1 : slope (torch's subgradient there is the same)
    _close(R.act_bwd_from_y(R.act(x, kind, slope), dy, kind, slope), want, "act_bwd_from_y")


@pytest.mark.parametrize("B,Z", [(1, 1), (3, 64), (5, 100)])
def test_latent(B, Z):
    g = _g(5)
    mu, eps = torch.randn(B, Z, generator=g).double(), torch.randn(B, Z, generator=g).double()
    lv = (torch.rand(B, Z, generator=g) * 10 - 6).double()
    dz, gkl = torch.randn(B, Z, generator=g).double(), torch.randn(B, generator=g).double()
    mr, lr_ = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)
    z = eps * torch.exp(0.5 * lr_) + mr
    kl = -0.5 * torch.sum(-lr_.exp() - torch.pow(mr, 2) + lr_ + 1, 1)
    ((z * dz).sum() + (kl * gkl).sum() + 0.25 * kl.sum()).backward()
    zr, klr = R.latent_fwd(mu, lv, eps)
    _close(zr, z.detach(), "z")
    _close(klr, kl.detach(), "kl")
    dmu, dlv = R.latent_bwd(mu, lv, eps, dz, gkl, 0.25)
    _close(dmu, mr.grad, "dmu")
    _close(dlv, lr_.grad, "dlogvar")
    # each term alone
    dmu0, dlv0 = R.latent_bwd(mu, lv, eps, dz, None, 0.0)
    _close(dmu0, dz, "dmu (dz only)")
    _close(dlv0, dz * eps * 0.5 * torch.exp(0.5 * lv), "dlogvar (dz only)")
    dmu1, dlv1 = R.latent_bwd(mu, lv, eps, None, gkl, 0.0)
    dmu2, dlv2 = R.latent_bwd(mu, lv, eps, None, None, 0.25)
    _close(dmu0 + dmu1 + dmu2, mr.grad, "dmu (sum of the parts)")
    _close(dlv0 + dlv1 + dlv2, lr_.grad, "dlogvar (sum of the parts)")


@pytest.mark.parametrize("n", [1, 2, 3, 5, 1027])
def test_bce(n):
    g = _g(6)
    p = (torch.rand(n, generator=g) * 0.98 + 0.01).double()
    t = torch.rand(n, generator=g).double()
    pr = p.clone().requires_grad_(True)
    s = F.binary_cross_entropy(pr, t, reduction="sum")
    (s * 0.7).backward()
    _close(R.bce_sum(p, t), s.detach(), "bce_sum")
    _close(R.bce_bwd(p, t, 0.35, 2.0), pr.grad, "bce_bwd")
    # dlogit of BCE(sigmoid(l), t) is p - t
    l = torch.randn(n, generator=g).double().requires_grad_(True)
    F.binary_cross_entropy(torch.sigmoid(l), t, reduction="sum").mul(0.3).backward()
    _close(R.bce_sigmoid_bwd(torch.sigmoid(l.detach()), t, 0.3), l.grad, "bce_sigmoid_bwd")
    # the clamp: p in {0, 1} at both ends
    if n >= 5:
        p[0], p[1], p[-2], p[-1] = 0.0, 1.0, 0.0, 1.0
        _close(R.bce_sum(p, t), F.binary_cross_entropy(p, t, reduction="sum"), "bce_sum (clamped)")
        d = R.bce_bwd(p, t)
        assert torch.isfinite(d).all() and d[0].item() == -t[0].item() / 1e-12


def test_bce_pad_and_vae_loss():
    g = _g(7)
    p, t = torch.rand(35, 3, generator=g).double(), torch.rand(35, 3, generator=g).double()
    pad = R.bce_sigmoid_bwd_pad(p, t, 0.5, 8)
    assert pad.shape == (35, 8) and (pad[:, 3:] == 0).all()
    _close(pad[:, :3], 0.5 * (p - t), "pad")
    kl = torch.randn(100, generator=g).double()
    recon, kl_sum, loss = R.vae_loss(p, t, kl, 0.01)
    want = F.binary_cross_entropy(p, t, reduction="sum")
    _close(recon, want, "recon")
    _close(kl_sum, kl.sum(), "kl_sum")
    _close(loss, (want + kl.sum()) / 100, "loss")
    x = torch.randn(1027, generator=g)
    _close(R.tensor_sum(x), x.double().sum(), "sum")
    _close(R.abs_sum(x), x.double().abs().sum(), "abs sum")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 1100])
def test_half_sqdiff(n):
    g = _g(8)
    a, b = torch.randn(3, n, generator=g).double(), torch.randn(3, n, generator=g).double()
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    e = 0.5 * (ar - br) ** 2
    ge, gr = torch.randn(3, n, generator=g).double(), torch.randn(3, generator=g).double()
    (e * ge).sum().backward()
    _close(R.half_sqdiff(a, b), e.detach(), "half_sqdiff")
    _close(R.half_sqdiff_rowsum(a, b), torch.sum(e.detach(), 1), "rowsum")
    da, db = R.half_sqdiff_bwd(a, b, ge, False)
    _close(da, ar.grad, "da")
    _close(db, br.grad, "db")
    ar.grad = br.grad = None
    (torch.sum(0.5 * (ar - br) ** 2, 1) * gr).sum().backward()
    da, db = R.half_sqdiff_bwd(a, b, gr, True)
    _close(da, ar.grad, "da per row")
    _close(db, br.grad, "db per row")


@pytest.mark.parametrize("B", [1, 5, 64, 100])
def test_gan_head_against_vaegan_loss(B):
    from oracle import ref_vaegan
    g = _g(9)
    logit = (torch.randn(3 * B, generator=g) * 3).double()
    if B > 1:      # autograd forms 1 - sigmoid(30) by subtraction and keeps three digits of it: invisible next to the other elements'
        logit[0], logit[B], logit[2 * B] = -30.0, 30.0, 30.0      # gradients, but all there is when B = 1
    lr_ = logit.clone().requires_grad_(True)
    dc = torch.sigmoid(lr_)
    z = torch.zeros(B, 1, dtype=torch.float64)
    _, _, _, bo, bp, bs, _ = ref_vaegan.vaegan_loss(z, z, z, z, z, dc[:B], dc[B:2 * B], dc[2 * B:], z, z, z, z)
    (1.7 * (bo.sum() + bp.sum() + bs.sum())).backward()
    p, sums, dl = R.gan_head(logit, B, 1.7)
    _close(p, dc.detach(), "p")
    _close(sums, torch.stack([bo.sum(), bp.sum(), bs.sum()]).detach(), "sums")
    _close(dl, lr_.grad, "dlogit")


def test_gan_head_saturated_logits_against_50_digits():
    """B = 1 with every logit saturated (-30 | 30 | 30), where torch's float64 autograd keeps three digits of 1 - sigmoid(30): the
    formula of the kernel comment, -log(p + 1e-3) | -log(1 - p + 1e-3) and coef times its derivative, in 50-digit decimal arithmetic"""
    from decimal import Decimal, getcontext
    getcontext().prec = 50
    coef, c = 1.7, Decimal("1e-3")
    p_, sums_, d_ = [], [], []
    for grp, x in enumerate((-30.0, 30.0, 30.0)):
        p = 1 / (1 + Decimal(-x).exp())
        u = (p if grp == 0 else 1 - p) + c
        p_.append(float(p))
        sums_.append(float(-u.ln()))
        d_.append(float(Decimal(coef) * (-1 if grp == 0 else 1) / u * p * (1 - p)))
    p, sums, dl = R.gan_head(torch.tensor([-30.0, 30.0, 30.0]), 1, coef)
    for name, got, want in (("p", p, p_), ("sums", sums, sums_), ("dlogit", dl, d_)):
        rel = ((got - torch.tensor(want, dtype=torch.float64)).abs() / torch.tensor(want, dtype=torch.float64).abs()).max().item()
        assert rel <= TOL, f"{name}: {got.tolist()} vs {want}: {rel:.3e}"      # every element relative to itself


@pytest.mark.parametrize("B,n1,n2", [(4, 3, 2), (1, 1, 0), (37, 5, 3)])
def test_smooth_l1_cat(B, n1, n2):
    from oracle import ref_vaegan
    g = _g(10)
    a = torch.randn(B, n1, generator=g).double()
    b = torch.randn(B, n2, generator=g).double() if n2 else None
    cat = a if b is None else torch.cat([a, b], 1)
    t = cat + torch.randn(B, n1 + n2, generator=g).double() * 1.5
    t[0, 0] = cat[0, 0] + 1.0
    if B > 1:
        t[1, -1] = cat[1, -1] - 1.0
    ar = a.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if n2 else None
    catr = ar if br is None else torch.cat([ar, br], 1)
    want = F.smooth_l1_loss(t, catr, reduction="sum") / B
    x = torch.zeros(B, 1, dtype=torch.float64)
    assert ref_vaegan.vaegan_loss(x, x, x, x, x, x + 0.5, x + 0.5, x + 0.5, x, x, t, catr)[6].item() == want.item()
    want.backward()
    loss, da, db = R.smooth_l1_cat(t, a, b, 1.0 / B)
    _close(loss, want.detach(), "loss")
    _close(da, ar.grad, "da")
    if n2:
        _close(db, br.grad, "db")
    else:
        assert db is None


@pytest.mark.parametrize("B,n", [(1, 1), (3, 8229)])
def test_be_and_dice_loss(B, n):
    from oracle import ref_be
    g = _g(11)
    x = (torch.randn(B, n, generator=g) * 3).double()
    t = (torch.rand(B, n, generator=g) < 0.4).double()
    xr = x.clone().requires_grad_(True)
    want = ref_be.be_loss(xr, t)
    (want * 1.3).backward()
    loss, sums, dx = R.be_loss(x, t, 0.5, 1.0, 1.3)
    _close(loss, want.detach(), "be loss")
    _close(dx, xr.grad, "be dx")
    p = torch.sigmoid(x)
    _close(sums[:, 0], F.binary_cross_entropy_with_logits(x, t, reduction="none").sum(1), "sum bce")
    _close(sums[:, 1:], torch.stack([(p * t).sum(1), p.sum(1), t.sum(1)], 1), "I, P, T")
    pr = (torch.rand(B, n, generator=g) * 0.98 + 0.01).double().requires_grad_(True)
    want = ref_be.dice_loss(pr, t, smooth=1.0)
    (want * 0.6).backward()
    loss, sums, dp = R.dice_loss(pr.detach(), t, 1.0, 0.6)
    _close(loss, want.detach(), "dice loss")
    _close(dp, pr.grad, "dice dp")
    assert (sums[:, 0] == 0).all()
    _close(sums[:, 1:], torch.stack([(pr.detach() * t).sum(1), pr.detach().sum(1), t.sum(1)], 1), "dice I, P, T")


@pytest.mark.parametrize("B,HW,C", [(2, 1, 3), (1, 3, 64), (3, 5, 130)])
def test_global_avgpool(B, HW, C):
    g = _g(12)
    x = torch.randn(B, HW, C, generator=g).double().requires_grad_(True)
    y = F.adaptive_avg_pool2d(x.permute(0, 2, 1).reshape(B, C, HW, 1), (1, 1)).reshape(B, C)
    dy = torch.randn(B, C, generator=g).double()
    y.backward(dy)
    _close(R.global_avgpool_fwd(x), y.detach(), "avgpool")
    _close(R.global_avgpool_bwd(dy, HW), x.grad, "avgpool bwd")


@pytest.mark.parametrize("Rr,n", [(1, 1), (5, 9), (7, 64), (6, 65), (7, 200)])
def test_softmax_rows(Rr, n):
    g = _g(13)
    x = (torch.randn(Rr, n, generator=g) * 20).double()
    x[Rr - 1] = 3.25
    xr = x.clone().requires_grad_(True)
    y = torch.softmax(xr, dim=-1)
    dy = torch.randn(Rr, n, generator=g).double()
    y.backward(dy)
    _close(R.softmax_rows_fwd(x), y.detach(), "softmax")
    _close(R.softmax_rows_bwd(y.detach(), dy), xr.grad, "softmax bwd")


@pytest.mark.parametrize("n", [1, 255, 257])
def test_l1_mean(n):
    g = _g(14)
    a, b = torch.randn(n, generator=g).double(), torch.randn(n, generator=g).double()
    b[::7] = a[::7]
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    want = F.l1_loss(ar, br)
    (want * 2.5).backward()
    _close(R.l1_mean(a, b), want.detach(), "l1")
    da, db = R.l1_mean_bwd(a, b, 2.5)
    assert (da[::7] == 0).all() and (db[::7] == 0).all()
    _close(da, ar.grad, "da")
    _close(db, br.grad, "db")


@pytest.mark.parametrize("B,C,H,W", [(1, 1, 1, 1), (2, 3, 1, 5), (1, 2, 4, 1), (2, 5, 7, 9)])
def test_upsample2x(B, C, H, W):
    g = _g(15)
    x = torch.randn(B, H, W, C, generator=g).double()
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=False)
    dy = torch.randn(B, 2 * H, 2 * W, C, generator=g).double()
    y.backward(dy.permute(0, 3, 1, 2))
    up, adj = R.upsample2x_fwd(x), R.upsample2x_bwd(dy)
    _close(up, y.detach().permute(0, 2, 3, 1), "upsample")
    _close(adj, xr.grad.permute(0, 2, 3, 1), "upsample adjoint")
    lhs, rhs = (up * dy).sum().item(), (x * adj).sum().item()
    scale = (up.abs() * dy.abs()).sum().item()
    assert abs(lhs - rhs) <= TOL * scale, f"<up(x), dy> = {lhs!r} but <x, up^T(dy)> = {rhs!r}"


@pytest.mark.parametrize("n", [1, 7, 1027])
def test_flat_optimisers(n):
    g = _g(16)
    lr, b1, b2, eps, alpha, gs = 1e-3, 0.9, 0.999, 1e-8, 0.99, 0.25
    p0 = torch.randn(n, generator=g).double()
    grads = [torch.randn(n, generator=g).double() for _ in range(2)]
    # torch starts from zero state; the reference is also stepped from the state torch holds after step 1 (non-zero m, v)
    pa = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pa], lr=lr, betas=(b1, b2), eps=eps)
    p, m, v = p0, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step, gr in enumerate(grads, 1):
        pa.grad = gr * gs
        opt.step()
        p, m, v = R.adam_step(p, gr, m, v, lr, b1, b2, eps, step, gs)
        st = opt.state[pa]
        _close(p, pa.detach(), f"adam p step {step}")
        _close(m, st["exp_avg"], f"adam m step {step}")
        _close(v, st["exp_avg_sq"], f"adam v step {step}")
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.RMSprop([pr], lr=lr, alpha=alpha, eps=eps)
    p, sq = p0, torch.zeros(n, dtype=torch.float64)
    for step, gr in enumerate(grads, 1):
        pr.grad = gr * gs
        opt.step()
        p, sq = R.rmsprop_step(p, gr, sq, lr, alpha, eps, gs)
        _close(p, pr.detach(), f"rmsprop p step {step}")
        _close(sq, opt.state[pr]["square_avg"], f"rmsprop sq step {step}")
