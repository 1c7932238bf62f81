"""float64 restatement of csrc/seg_eval.hip (every output of vp_seg_eval_f32), the two seeded input families its tests use, the
hand-made edge cases, and the planted faults that show the cases can tell a wrong kernel from a right one.  CPU only.

Inputs are (heads, B, 1, H, W) or (n, 1, H, W) fp32 tensors; the bits are taken from the fp32 values against fp32 thresholds, as the
kernel takes them, the sums from the values widened to float64."""
import torch
import torch.nn.functional as F

FAULTS = ("wrap", "image_leak", "head_leak", "drop_tail", "nan_pred", "gt")
SHAPES = ((1, 1, 1, 1), (1, 2, 5, 7), (2, 3, 12, 20), (1, 1, 33, 130), (2, 2, 64, 64))      # (heads, B, H, W)


# ---- input families ------------------------------------------------------------------------------------------------------------------
def ring(seed, heads, B, H, W):
    """target: a ring of half-width 0.8 px around a random centre; logits: 4 (1 - |d' - r|) + 0.5 + 1.5 randn on the same ring shifted
    by (+1, -1) px, so prediction and target overlap in part and the rest lies one pixel off"""
    g = torch.Generator().manual_seed(seed)
    n = heads * B
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    cy = (H - 1) * (0.3 + 0.4 * torch.rand(n, 1, 1, generator=g, dtype=torch.float64))
    cx = (W - 1) * (0.3 + 0.4 * torch.rand(n, 1, 1, generator=g, dtype=torch.float64))
    r = 1.0 + 0.3 * min(H, W) * torch.rand(n, 1, 1, generator=g, dtype=torch.float64)
    d = ((yy - cy) ** 2 + (xx - cx) ** 2).sqrt()
    ds = ((yy - cy - 1) ** 2 + (xx - cx + 1) ** 2).sqrt()
    targets = ((d - r).abs() <= 0.8).float()
    logits = (4 * (1 - (ds - r).abs()) + 0.5 + 1.5 * torch.randn(n, H, W, generator=g, dtype=torch.float64)).float()
    return logits.view(heads, B, 1, H, W), targets.view(heads, B, 1, H, W)


def sparse(seed, heads, B, H, W):
    """target bits Bernoulli(0.03) (0.08 below 100 pixels); logits +-3 + 0.5 randn, positive with the same density, independently"""
    g = torch.Generator().manual_seed(seed)
    density = 0.08 if H * W < 100 else 0.03
    shape = (heads, B, 1, H, W)
    targets = (torch.rand(shape, generator=g) < density).float()
    sign = (torch.rand(shape, generator=g) < density).float() * 2 - 1
    return 3 * sign + 0.5 * torch.randn(shape, generator=g), targets


FAMILIES = {"ring": ring, "sparse": sparse}


def case(family, shape, seed=0):
    return FAMILIES[family](1000 * seed + 17 * shape[2] + shape[3], *shape)


def explicit_cases():
    """name -> (logits, targets, tol): one bit of P and one of T each, placed where only a wrong window finds the other"""
    def planes(heads, B, H, W, p_at, t_at):
        x, t = torch.full((heads, B, 1, H, W), -3.0), torch.zeros((heads, B, 1, H, W))
        x[p_at[0], p_at[1], 0, p_at[2], p_at[3]] = 3.0
        t[t_at[0], t_at[1], 0, t_at[2], t_at[3]] = 1.0
        return x, t
    out = {"wrap": planes(1, 1, 4, 6, (0, 0, 1, 5), (0, 0, 2, 0)) + (1,),               # P at (r, W-1), T at (r+1, 0)
           "image_leak": planes(1, 2, 4, 6, (0, 0, 3, 2), (0, 1, 0, 2)) + (1,),         # P in the last row of image 0, T in the first of image 1
           "head_leak": planes(2, 1, 4, 6, (0, 0, 3, 2), (1, 0, 0, 2)) + (1,),          # ... of head 0's last image, head 1's first
           "tail": planes(1, 1, 5, 7, (0, 0, 4, 6), (0, 0, 4, 5)) + (0,)}               # 35 pixels: the last three are a partial vector
    x, t = planes(1, 1, 3, 8, (0, 0, 1, 1), (0, 0, 1, 1))
    x[0, 0, 0, 2, 3], t[0, 0, 0, 2, 3] = float("nan"), 1.0
    out["nan"] = (x, t, 0)
    x, t = planes(1, 1, 3, 8, (0, 0, 1, 1), (0, 0, 1, 1))
    x[0, 0, 0, 0, 4:] = 0.5                                                             # exactly the threshold: predicted
    out["at_threshold"] = (x, t, 1)
    return out


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def _dilate(bits, tol, fault):
    """bits (heads, B, H, W) as float; OR over the (2 tol + 1)^2 window clipped to the image"""
    heads, B, H, W = bits.shape
    if tol == 0:
        return bits
    k = 2 * tol + 1
    if fault == "wrap":                  # the row's window runs on into the neighbouring rows
        flat = F.max_pool1d(bits.reshape(heads * B, 1, H * W), k, stride=1, padding=tol).reshape(heads * B, 1, H, W)
        return F.max_pool2d(flat, (k, 1), stride=1, padding=(tol, 0)).reshape(heads, B, H, W)
    if fault == "image_leak":            # the images of a head stacked into one tall plane
        return F.max_pool2d(bits.reshape(heads, 1, B * H, W), k, stride=1, padding=tol).reshape(heads, B, H, W)
    if fault == "head_leak":             # the last image of a head and the first of the next share a border
        out = F.max_pool2d(bits.reshape(heads * B, 1, H, W), k, stride=1, padding=tol).reshape(heads, B, H, W).clone()
        tall = F.max_pool2d(bits.reshape(1, 1, heads * B * H, W), k, stride=1, padding=tol).reshape(heads, B, H, W)
        for h in range(heads - 1):
            out[h, B - 1], out[h + 1, 0] = tall[h, B - 1], tall[h + 1, 0]
        return out
    return F.max_pool2d(bits.reshape(heads * B, 1, H, W), k, stride=1, padding=tol).reshape(heads, B, H, W)


def reference(logits, targets, threshold=0.5, tol=0, bce_weight=0.5, smooth=1.0, target_threshold=0.5, fault=None):
    """{"sums" (n, 4) float64, "terms" (n, 3) float64, "counts" (n, 6) int64}, n = heads * B images in the kernel's order"""
    assert fault is None or fault in FAULTS
    x5 = logits if logits.dim() == 5 else logits[None]
    t5 = targets if targets.dim() == 5 else targets[None]
    heads, B, _, H, W = x5.shape
    n = heads * B
    xf, tf = x5.reshape(heads, B, H, W).float().cpu(), t5.reshape(heads, B, H, W).float().cpu()
    thr, tthr = torch.tensor(threshold, dtype=torch.float32), torch.tensor(target_threshold, dtype=torch.float32)
    P = xf > thr if fault == "gt" else ~(xf < thr) if fault == "nan_pred" else xf >= thr
    T = tf >= tthr
    if fault == "drop_tail" and (H * W) % 4:
        keep = torch.ones(H * W, dtype=torch.bool)
        keep[H * W - (H * W) % 4:] = False
        P, T = P & keep.view(H, W), T & keep.view(H, W)
    Pd, Td = _dilate(P.float(), tol, fault) > 0, _dilate(T.float(), tol, fault) > 0
    per = lambda m: m.reshape(n, -1).sum(1)                                        # noqa: E731
    counts = torch.stack([per(P), per(T), per(P & T), per(P & Td), per(T & Pd), per(~torch.isfinite(xf))], 1).long()
    x, t = xf.double().reshape(n, -1), tf.double().reshape(n, -1)
    p = torch.sigmoid(x)
    bce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    sums = torch.stack([bce.sum(1), (p * t).sum(1), p.sum(1), t.sum(1)], 1)
    mean_bce = sums[:, 0] / (H * W)
    dice = (2 * sums[:, 1] + smooth) / (sums[:, 2] + sums[:, 3] + smooth)
    return {"sums": sums, "terms": torch.stack([mean_bce, dice, bce_weight * mean_bce + 1 - dice], 1), "counts": counts}
