"""fp64 direct sums of the three k x k convolution families (ks in {1, 3, 5}, stride 1 or 2, padding (ks - 1) // 2), straight from
their definition, at sampled output elements -- the reference the kernels' outputs are held to at launch shapes where a whole fp64
convolution would be too slow (tests/test_gpu_properties.py, tests/test_gpu_wgrad_budget.py, tests/test_gpu_conv_direct_kxk.py).

Weights are in the reference layout w[cs][cb][r][q] (Cs small-side channels, Cb big-side channels; nn.Conv2d(Cb -> Cs) weight,
nn.ConvTranspose2d(Cs -> Cb) weight), activations are logical NCHW tensors in any memory layout on any device.  With s = stride and
p = padding the small side is Hs = floor((Hb + 2p - ks) / s) + 1 (the rule conv_check of csrc/conv.hip enforces: with stride 2 and an
odd Hb the big side is not 2 * Hs):

  gather   small[b, cs, h, x] = sum_{cb, r, q} w[cs, cb, r, q] * big[b, cb, s*h - p + r, s*x - p + q]
  scatter  big[b, cb, y, x]   = sum_{cs, r, q : y = s*h - p + r, x = s*v - p + q} w[cs, cb, r, q] * small[b, cs, h, v]
  wgrad    dW[cs, cb, r, q]   = sum_{b, h, v} small[b, cs, h, v] * big[b, cb, s*h - p + r, s*v - p + q]

(out-of-range big pixels are zero).  The kernel size is the weight's; the stride defaults to 2, so the 5x5 calls of the VAE layers
read as before.  Each function returns, per sampled element, r = sum a_i b_i and A = sum |a_i b_i| in float64 -- and with
``terms=True`` also K, the number of terms of the sum: A bounds what the rounding of the terms can do, so a kernel result `out` is
checked as |out - r| <= tau(K) * A.  Only the operand elements a sample needs are gathered (advanced indexing on the device) before
the conversion to float64; no library kernel is called.
"""
import torch

PAD, STRIDE, KS = 2, 2, 5


def pad_of(ks):
    return (ks - 1) // 2


def out_size(n, ks=KS, stride=STRIDE):
    """small-side extent of a big side n: floor((n + 2p - ks) / stride) + 1"""
    return (n + 2 * pad_of(ks) - ks) // stride + 1


def _seeded_image(B, seed):
    return int(torch.randint(0, B, (1,), generator=torch.Generator().manual_seed(seed)).item())


def gather_points(B, Hs, seed, Ws=None):
    """(b, h, x) samples of the gather output: rows {0, 1, Hs/2, Hs-2, Hs-1} x columns {0, 1, Ws/2, Ws-2, Ws-1} (both borders and the
    middle; Ws defaults to Hs) of images {0, B-1, one seeded random image}"""
    Ws = Hs if Ws is None else Ws
    imgs = sorted({0, B - 1, _seeded_image(B, seed)})
    rows = sorted({v for v in (0, 1, Hs // 2, Hs - 2, Hs - 1) if 0 <= v < Hs})
    cols = sorted({v for v in (0, 1, Ws // 2, Ws - 2, Ws - 1) if 0 <= v < Ws})
    return [(b, h, x) for b in imgs for h in rows for x in cols]


def _scatter_lines(n):
    # both parities at both borders and in the middle; an odd side also gets n - 3, so that the last three lines -- the last of which
    # the stride-2 scatter reaches with fewer taps -- are all sampled
    lines = {0, 1, 2, 3, n // 2, n // 2 + 1, n - 2, n - 1} | ({n - 3} if n % 2 else set())
    return sorted(v for v in lines if 0 <= v < n)


def scatter_points(B, Hb, seed, Wb=None):
    """(b, y, x) samples of the scatter output: rows and columns {0, 1, 2, 3, Hb/2, Hb/2+1, Hb-2, Hb-1} (and Hb-3 for an odd side)
    -- both parities in both dimensions (all four phases of the stride-2 decomposition) at both borders and in the middle"""
    Wb = Hb if Wb is None else Wb
    imgs = sorted({0, B - 1, _seeded_image(B, seed)})
    return [(b, y, x) for b in imgs for y in _scatter_lines(Hb) for x in _scatter_lines(Wb)]


def edge_channels(C):
    """channel indices at the edges of 64- and 128-wide tiles: {0, 63, 64, 127, 128, C-1}, those that exist"""
    return sorted({c for c in (0, 63, 64, 127, 128, C - 1) if 0 <= c < C})


def tile_channels(C):
    """channel indices at the edges of 8-, 16-, 32-, 64- and 128-wide tiles and the last channel: for a channel count that the front
    end zero-pads to a multiple of 8, C - 1 is the last real channel"""
    return sorted({c for c in (0, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, C - 1) if 0 <= c < C})


def _idx(pts, device):
    t = torch.tensor(pts, dtype=torch.long, device=device)
    return t[:, 0], t[:, 1], t[:, 2]


def _contract(vals, w):
    """vals (n, ks, ks, C) float64 operand values per tap, w (C, D, ks, ks) -> r, A of shape (n, D)"""
    wd = w.detach().double()
    r = torch.einsum("nrqc,cdrq->nd", vals, wd)
    A = torch.einsum("nrqc,cdrq->nd", vals.abs(), wd.abs())
    return r, A


def _gather_taps(h, n_big, ks, stride):
    """big line of tap r for small line h, and whether it exists: (n, ks) each"""
    tap = torch.arange(ks, device=h.device)
    yy = (stride * h - pad_of(ks))[:, None] + tap[None, :]
    return yy.clamp(0, n_big - 1), (yy >= 0) & (yy < n_big)


def gather_ref(big, w, pts, stride=STRIDE, terms=False):
    """r, A (len(pts), Cs) of the gather small[b, :, h, x] for (b, h, x) in pts; big (B, Cb, Hb, Wb), w (Cs, Cb, ks, ks)"""
    _, Cb, Hb, Wb = big.shape
    ks = w.shape[-1]
    b, h, x = _idx(pts, big.device)
    yc, oky = _gather_taps(h, Hb, ks, stride)
    xc, okx = _gather_taps(x, Wb, ks, stride)
    ok = oky[:, :, None] & okx[:, None, :]
    vals = big[b[:, None, None], :, yc[:, :, None], xc[:, None, :]]      # (n, ks, ks, Cb), only the patches
    vals = vals.double() * ok[..., None]
    r, A = _contract(vals, w.permute(1, 0, 2, 3))
    return (r, A, (ok.sum((1, 2)) * Cb)[:, None].expand_as(r)) if terms else (r, A)


def _scatter_src(y, n_small, ks=KS, stride=STRIDE):
    """small line h feeding big line y through tap r (y = s*h - p + r), and whether that tap exists: (n, ks) each"""
    tap = torch.arange(ks, device=y.device)
    t = y[:, None] + pad_of(ks) - tap[None, :]
    ok = (t % stride == 0) & (t >= 0) & (t < stride * n_small)
    return (t // stride).clamp(0, n_small - 1), ok


def scatter_ref(small, w, pts, stride=STRIDE, terms=False):
    """r, A (len(pts), Cb) of the scatter big[b, :, y, x] for (b, y, x) in pts; small (B, Cs, Hs, Ws), w (Cs, Cb, ks, ks)"""
    _, Cs, Hs, Ws = small.shape
    ks = w.shape[-1]
    b, y, x = _idx(pts, small.device)
    hs, okh = _scatter_src(y, Hs, ks, stride)
    vs, okv = _scatter_src(x, Ws, ks, stride)
    ok = okh[:, :, None] & okv[:, None, :]
    vals = small[b[:, None, None], :, hs[:, :, None], vs[:, None, :]]    # (n, ks, ks, Cs)
    vals = vals.double() * ok[..., None]
    r, A = _contract(vals, w)
    return (r, A, (ok.sum((1, 2)) * Cs)[:, None].expand_as(r)) if terms else (r, A)


def scatter_terms(pts, Hs, Ws, Cs, ks=KS, stride=STRIDE):
    """number of terms of each scatter sample (taps that exist x Cs): for the 5x5 stride-2 layers from 9 * Cs in the interior down to
    Cs at the far corner (Hb - 1, Wb - 1), which only tap (3, 3) reaches"""
    b, y, x = _idx(pts, "cpu")
    return _scatter_src(y, Hs, ks, stride)[1].sum(1) * _scatter_src(x, Ws, ks, stride)[1].sum(1) * Cs


def wgrad_ref(big, small, cs_list, cb_list, ks=KS, stride=STRIDE, terms=False):
    """r, A (len(cs_list), len(cb_list), ks, ks) of dW[cs, cb, :, :]: for each channel pair the full sum over all B * Hs * Ws pixels"""
    B, _, Hb, Wb = big.shape
    _, _, Hs, Ws = small.shape
    p = pad_of(ks)
    dev = big.device
    s = small[:, torch.tensor(cs_list, device=dev)].double()              # (B, ns, Hs, Ws): only the sampled channels
    g = big[:, torch.tensor(cb_list, device=dev)].double()                # (B, nb, Hb, Wb)
    g = torch.nn.functional.pad(g, (p, p, p, p))                          # zero border: padded line s*h + r = big line s*h - p + r
    r = torch.empty(len(cs_list), len(cb_list), ks, ks, dtype=torch.float64, device=dev)
    A = torch.empty_like(r)
    for i in range(ks):
        for j in range(ks):
            t = g[:, :, i:i + stride * (Hs - 1) + 1:stride, j:j + stride * (Ws - 1) + 1:stride]
            r[:, :, i, j] = torch.einsum("bshw,bchw->sc", s, t)
            A[:, :, i, j] = torch.einsum("bshw,bchw->sc", s.abs(), t.abs())
    if not terms:
        return r, A
    ky = (_gather_taps(torch.arange(Hs), Hb, ks, stride)[1]).sum(0)       # (ks,): small rows whose tap r lands inside the big side
    kx = (_gather_taps(torch.arange(Ws), Wb, ks, stride)[1]).sum(0)
    K = (B * ky[:, None] * kx[None, :]).to(dev)
    return r, A, K.expand_as(r)


def take(out, pts):
    """kernel output out (B, C, H, W) at the sampled pixels, as (len(pts), C) float64"""
    b, h, x = _idx(pts, out.device)
    return out[b, :, h, x].double()


def worst(got, r, A):
    """max over the samples of |got - r| / A (A = 0, an all-zero sum, counts as 1) and the flat index of that sample"""
    e = (got.double() - r).abs() / torch.where(A > 0, A, torch.ones_like(A))
    i = int(e.flatten().argmax().item())
    return e.flatten()[i].item(), i


def worst_scaled(got, r, A, tau):
    """max over the samples of |got - r| / (tau * A), tau a tensor of per-sample tolerances broadcastable to r (A = 0 counts as 1),
    the flat index of that sample and its |got - r| / A"""
    e = (got.double() - r).abs() / torch.where(A > 0, A, torch.ones_like(A))
    s = e / tau
    i = int(s.flatten().argmax().item())
    return s.flatten()[i].item(), i, e.flatten()[i].item()


# ---- tolerances of a direct-sum check, from the arithmetic (fixed before any measurement) -------------------------------------------
# A sample is r = sum_i a_i b_i over K terms and A = sum |a_i b_i|.  The k x k layers break the K >= 392 premise of the TAU table in
# tests/test_gpu_properties.py: a 1x1 layer over 16 channels sums 16 terms, a border sample of a 3x3 layer with one input channel 4,
# the far corner of a 3x3 stride-2 scatter with 2 small channels 2.  So tau is a function of K:
#   tau(K, mode) = SAFETY * (min(1.6, K) * u  +  m * d * min(1, 1.57 / sqrt(K)))
#   - u = 2^-24: the fp32 accumulation, |out - r| / A ~ 1.6 u for random rounding (tests/test_gpu_properties.py), and never more than
#     K u -- one rounding per term -- for tiny K;
#   - m operands per product rounded with a relative error of rms d: for Gaussian operands sqrt(sum (a_i b_i)^2) / A = 1.57 / sqrt(K),
#     so random rounding gives m d 1.57 / sqrt(K); that estimate exceeds the deterministic worst case m d (every term off by d in the
#     same direction) for K <= 2, where the worst case is used;
#   - SAFETY = 10, as the rounding from the estimate to the table of tests/test_gpu_properties.py (f32 1.6 u -> 1e-6).
#     mode              m  d                                                              tau(392)   tau(16)    tau(4)
#     f32, small3       0  -  (exact fp32 products: the fp32 MFMA and VALU kernels)       9.5e-7     9.5e-7     9.5e-7
#     bf16x3            2  2^-17 (hi + lo keep 16 bits; the dropped lo * lo is < 2^-18)   1.3e-5     6.1e-5     1.2e-4
#     f16x2/3           2  2^-20 (hi + lo keep 22 bits, as the existing table)            2.5e-6     8.4e-6     1.6e-5
#     f16x2/2           1  2.1e-4 (one operand keeps its fp16 hi plane only)              1.7e-4     8.2e-4     1.6e-3
#     f16x2/2 declared: as f16x2/3, against the operation with that operand rounded to fp16 (its declared arithmetic)
# A failure is a finding to explain, never a reason to raise tau.
SAFETY = 10.0
U32 = 2.0 ** -24
_ROUNDED = {"f32": (0, 0.0), "small3": (0, 0.0), "bf16x3": (2, 2.0 ** -17), "f16x2/3": (2, 2.0 ** -20), "f16x2/2": (1, 2.1e-4),
            "f16x2/2 declared": (2, 2.0 ** -20)}


def tau(K, mode):
    """tolerance on |out - r| / A of a K-term sample in arithmetic `mode` (the derivation above); K a number or a tensor"""
    m, d = _ROUNDED[mode]
    K = torch.as_tensor(K, dtype=torch.float64).clamp(min=1)
    return SAFETY * (K.clamp(max=1.6) * U32 + m * d * (1.57 / K.sqrt()).clamp(max=1.0))
