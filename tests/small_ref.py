"""fp64 references of the small kernels of csrc/elementwise.hip and of the two activation kernels of csrc/bn.hip, written from the
definitions in the kernels' header comments (include/vaeplay_hip.h) -- the reference the GPU tests of the loss, pointwise and
flat-optimiser entry points hold the kernels to (tests/test_gpu_small_losses.py, tests/test_gpu_small_pointwise.py,
tests/test_gpu_flat_optim.py); tests/test_small_ref_cpu.py checks every function here against torch's own float64 operator.

Every function takes fp32 (or any real) CPU tensors, converts them to float64, evaluates the formula and returns float64.  Nothing
here touches a device or a project kernel.  Activations are in the layout the kernels index: NHWC arrays [B, H, W, C] (or
[B, HW, C]), matrices [R, n], flat vectors.
"""
import math

import torch

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4


def D(t):
    return t.detach().to(device="cpu", dtype=torch.float64)


# ---- layout ---------------------------------------------------------------------------------------------------------------------
def nchw_to_nhwc(x):
    """[B, C, H, W] -> [B, H, W, C]"""
    return D(x).permute(0, 2, 3, 1).contiguous()


def nhwc_to_nchw(x):
    """[B, H, W, C] -> [B, C, H, W]"""
    return D(x).permute(0, 3, 1, 2).contiguous()


def slice_channels(x, Cout):
    """out[..., c] = x[..., c] for c < Cout"""
    return D(x)[..., :Cout].contiguous()


def add_coords(x, normalize):
    """AddCoords on [B, H, W, C]: channel C = column index, channel C + 1 = row index; normalised: (index / extent - 0.5) / 0.5"""
    x = D(x)
    B, H, W, C = x.shape
    ci = torch.arange(W, dtype=torch.float64).reshape(1, 1, W, 1).expand(B, H, W, 1)
    cj = torch.arange(H, dtype=torch.float64).reshape(1, H, 1, 1).expand(B, H, W, 1)
    if normalize:
        ci = (ci / W - 0.5) / 0.5
        cj = (cj / H - 0.5) / 0.5
    return torch.cat([x, ci, cj], dim=3)


# ---- activations ----------------------------------------------------------------------------------------------------------------
def act(x, kind, slope=0.0):
    x = D(x)
    if kind == ACT_RELU:
        return torch.where(x > 0, x, torch.zeros_like(x))
    if kind == ACT_LRELU:
        return torch.where(x > 0, x, x * slope)
    if kind == ACT_TANH:
        return torch.tanh(x)
    if kind == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-x))
    return x.clone()


def act_grad_from_y(y, kind, slope=0.0):
    """act'(.) expressed through the OUTPUT y"""
    y = D(y)
    one = torch.ones_like(y)
    if kind == ACT_RELU:
        return torch.where(y > 0, one, torch.zeros_like(y))
    if kind == ACT_LRELU:
        return torch.where(y > 0, one, one * slope)
    if kind == ACT_TANH:
        return 1.0 - y * y
    if kind == ACT_SIGMOID:
        return y * (1.0 - y)
    return one


def act_bwd_from_y(y, dy, kind, slope=0.0):
    return D(dy) * act_grad_from_y(y, kind, slope)


# ---- latent ---------------------------------------------------------------------------------------------------------------------
def latent_fwd(mu, logvar, eps):
    """z = eps * exp(0.5 logvar) + mu ; kl[b] = -0.5 sum_j (1 + logvar - mu^2 - exp(logvar))"""
    mu, lv, eps = D(mu), D(logvar), D(eps)
    z = eps * torch.exp(0.5 * lv) + mu
    kl = -0.5 * torch.sum(1.0 + lv - mu * mu - torch.exp(lv), dim=1)
    return z, kl


def latent_bwd(mu, logvar, eps, dz=None, gkl=None, gkl_scalar=0.0):
    """dmu = dz + g_b mu ; dlogvar = dz eps 0.5 exp(0.5 logvar) + g_b 0.5 (exp(logvar) - 1), g_b = gkl[b] + gkl_scalar"""
    mu, lv, eps = D(mu), D(logvar), D(eps)
    dz = torch.zeros_like(mu) if dz is None else D(dz)
    g = torch.full((mu.shape[0], 1), float(gkl_scalar), dtype=torch.float64)
    if gkl is not None:
        g = g + D(gkl).reshape(-1, 1)
    dmu = dz + g * mu
    dlv = dz * eps * 0.5 * torch.exp(0.5 * lv) + g * 0.5 * (torch.exp(lv) - 1.0)
    return dmu, dlv


# ---- BCE and plain sums ---------------------------------------------------------------------------------------------------------
def bce_terms(p, t):
    """-[t max(log p, -100) + (1 - t) max(log(1 - p), -100)] per element (torch's clamp of the two logs)"""
    p, t = D(p), D(t)
    lp = torch.clamp(torch.log(p), min=-100.0)
    lq = torch.clamp(torch.log(1.0 - p), min=-100.0)
    return -(t * lp + (1.0 - t) * lq)


def bce_sum(p, t):
    return bce_terms(p, t).sum()


def bce_bwd(p, t, g=1.0, gscale=1.0):
    """dp = g gscale (p - t) / max(p (1 - p), 1e-12)"""
    p, t = D(p), D(t)
    return float(g) * float(gscale) * (p - t) / torch.clamp((1.0 - p) * p, min=1e-12)


def bce_sigmoid_bwd(p, t, gscale):
    """dlogit = gscale (p - t)"""
    return float(gscale) * (D(p) - D(t))


def bce_sigmoid_bwd_pad(p, t, gscale, Cpad):
    """the same on [npix, C], zero-padded to [npix, Cpad]"""
    d = bce_sigmoid_bwd(p, t, gscale)
    npix, C = d.shape
    out = torch.zeros(npix, Cpad, dtype=torch.float64)
    out[:, :C] = d
    return out


def vae_loss(x_tilde, x, kl, loss_scale):
    """(recon, kl_sum, (recon + kl_sum) * loss_scale)"""
    recon = bce_sum(x_tilde, x)
    kl_sum = D(kl).sum()
    return recon, kl_sum, (recon + kl_sum) * float(loss_scale)


def tensor_sum(x):
    return D(x).sum()


def abs_sum(x):
    return D(x).abs().sum()


# ---- 0.5 (a - b)^2 --------------------------------------------------------------------------------------------------------------
def half_sqdiff(a, b):
    d = D(a) - D(b)
    return 0.5 * d * d


def half_sqdiff_rowsum(a, b):
    """a, b [R, n] -> [R]"""
    return half_sqdiff(a, b).sum(dim=1)


def half_sqdiff_bwd(a, b, g, per_row):
    """da = g (a - b), db = -da; a, b [R, n]; g [R] (per_row) or [R, n]"""
    a, b, g = D(a), D(b), D(g)
    g = g.reshape(-1, 1) if per_row else g.reshape(a.shape)
    da = g * (a - b)
    return da, -da


# ---- VAE-GAN loss heads ---------------------------------------------------------------------------------------------------------
def gan_head(logit, B, coef):
    """logit [3B] of (original | reconstructed | sampled): p = sigmoid; sums = (sum -log(p + 1e-3) over the originals,
    sum -log(1 - p + 1e-3) over the reconstructed, the same over the sampled); dlogit = coef d(sum of the three) / dlogit"""
    x = D(logit).reshape(3, B)
    p = 1.0 / (1.0 + torch.exp(-x))
    q = 1.0 / (1.0 + torch.exp(x))       # 1 - p, without the cancellation (a saturated logit keeps its digits in float64 too)
    u = torch.cat([p[:1] + 1e-3, q[1:] + 1e-3], dim=0)
    sums = (-torch.log(u)).sum(dim=1)
    dldp = torch.cat([-1.0 / u[:1], 1.0 / u[1:]], dim=0)
    dlogit = float(coef) * dldp * p * q
    return p.reshape(-1), sums, dlogit.reshape(-1)


def smooth_l1_cat(t, a, b, scale):
    """scale * sum smooth_l1(t - cat(a, b)) with beta = 1; (loss, da, db); b may be None (n2 = 0)"""
    t, a = D(t), D(a)
    pv = a if b is None else torch.cat([a, D(b)], dim=1)
    d = t - pv
    ad = d.abs()
    loss = float(scale) * torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5).sum()
    g = -float(scale) * torch.clamp(d, -1.0, 1.0)
    n1 = a.shape[1]
    return loss, g[:, :n1].contiguous(), (None if b is None else g[:, n1:].contiguous())


# ---- segmentation losses --------------------------------------------------------------------------------------------------------
def _dice_parts(p, t, smooth):
    I, P, T = (p * t).sum(dim=1), p.sum(dim=1), t.sum(dim=1)
    return I, P, T, P + T + smooth


def be_loss(x, t, bce_weight, smooth, g=1.0):
    """w * mean BCEWithLogits(x, t) + 1 - mean_b (2 I_b + s) / (P_b + T_b + s), p = sigmoid(x); x, t [B, n].
    (loss, sums [B, 4] = {sum bce, I, P, T}, dx = g dloss/dx)"""
    x, t = D(x), D(t)
    B, n = x.shape
    p = 1.0 / (1.0 + torch.exp(-x))
    bce = torch.clamp(x, min=0.0) - x * t + torch.log1p(torch.exp(-x.abs()))
    I, P, T, Dn = _dice_parts(p, t, smooth)
    sums = torch.stack([bce.sum(dim=1), I, P, T], dim=1)
    loss = bce_weight * bce.sum() / (B * n) + 1.0 - ((2.0 * I + smooth) / Dn).sum() / B
    ab = (-2.0 / (B * Dn)).reshape(-1, 1)
    bb = ((2.0 * I + smooth) / (B * Dn * Dn)).reshape(-1, 1)
    dx = float(g) * (bce_weight / (B * n) * (p - t) + (ab * t + bb) * p * (1.0 - p))
    return loss, sums, dx


def dice_loss(p, t, smooth, g=1.0):
    """1 - mean_b (2 I_b + s) / (P_b + T_b + s) on probabilities p; sums[b] = {0, I, P, T}; dp = g dloss/dp"""
    p, t = D(p), D(t)
    B = p.shape[0]
    I, P, T, Dn = _dice_parts(p, t, smooth)
    sums = torch.stack([torch.zeros_like(I), I, P, T], dim=1)
    loss = 1.0 - ((2.0 * I + smooth) / Dn).sum() / B
    ab = (-2.0 / (B * Dn)).reshape(-1, 1)
    bb = ((2.0 * I + smooth) / (B * Dn * Dn)).reshape(-1, 1)
    return loss, sums, float(g) * (ab * t + bb)


# ---- pooling, softmax, L1 -------------------------------------------------------------------------------------------------------
def global_avgpool_fwd(x):
    """[B, HW, C] -> [B, C] means over the pixels"""
    return D(x).mean(dim=1)


def global_avgpool_bwd(dy, HW):
    """[B, C] -> [B, HW, C]: dy / HW at every pixel"""
    dy = D(dy)
    return (dy / HW).unsqueeze(1).expand(dy.shape[0], HW, dy.shape[1]).contiguous()


def softmax_rows_fwd(x):
    x = D(x)
    e = torch.exp(x - x.max(dim=1, keepdim=True).values)
    return e / e.sum(dim=1, keepdim=True)


def softmax_rows_bwd(y, dy):
    """dx = y (dy - sum_j dy_j y_j)"""
    y, dy = D(y), D(dy)
    return y * (dy - (dy * y).sum(dim=1, keepdim=True))


def l1_mean(a, b):
    return (D(a) - D(b)).abs().mean()


def l1_mean_bwd(a, b, g=1.0):
    """da = sign(a - b) g / n (0 where a == b), db = -da"""
    d = D(a) - D(b)
    da = torch.sign(d) * (float(g) / d.numel())
    return da, -da


# ---- 2x bilinear upsample (align_corners=False) ---------------------------------------------------------------------------------
def _bilinear_matrix(n):
    """[2n, n]: row o holds the two weights of src = max((o + 0.5) / 2 - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, n - 1)"""
    M = torch.zeros(2 * n, n, dtype=torch.float64)
    for o in range(2 * n):
        src = max((o + 0.5) * 0.5 - 0.5, 0.0)
        i0 = int(src)
        i1 = min(i0 + 1, n - 1)
        lam = src - i0
        M[o, i0] += 1.0 - lam
        M[o, i1] += lam
    return M


def upsample2x_fwd(x):
    """[B, H, W, C] -> [B, 2H, 2W, C]"""
    x = D(x)
    MH, MW = _bilinear_matrix(x.shape[1]), _bilinear_matrix(x.shape[2])
    return torch.einsum("pw,bowc->bopc", MW, torch.einsum("oh,bhwc->bowc", MH, x)).contiguous()


def upsample2x_bwd(dy):
    """the adjoint: [B, 2H, 2W, C] -> [B, H, W, C]"""
    dy = D(dy)
    MH, MW = _bilinear_matrix(dy.shape[1] // 2), _bilinear_matrix(dy.shape[2] // 2)
    return torch.einsum("pw,bhpc->bhwc", MW, torch.einsum("oh,bopc->bhpc", MH, dy)).contiguous()


# ---- flat optimiser steps -------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """torch.optim.Adam (no amsgrad, no weight decay), step 1-based: gr = g grad_scale; m += (1 - b1)(gr - m);
    v = v b2 + (1 - b2) gr^2; p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps).  Returns (p, m, v)."""
    p, m, v = D(p), D(m), D(v)
    gr = D(g) * float(grad_scale)
    m = m + (1.0 - beta1) * (gr - m)
    v = v * beta2 + (1.0 - beta2) * gr * gr
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = torch.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def rmsprop_step(p, g, sq, lr, alpha, eps, grad_scale=1.0):
    """torch.optim.RMSprop (no momentum, not centered): sq = alpha sq + (1 - alpha) gr^2; p -= lr gr / (sqrt(sq) + eps)"""
    p, sq = D(p), D(sq)
    gr = D(g) * float(grad_scale)
    sq = sq * alpha + (1.0 - alpha) * gr * gr
    return p - lr * (gr / (torch.sqrt(sq) + eps)), sq
