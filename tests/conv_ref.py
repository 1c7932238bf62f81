"""fp64 direct sums of the three 5x5 / padding-2 / stride-2 convolution families, straight from their definition, at sampled
output elements -- the reference the kernels' outputs are held to at launch shapes where a whole fp64 convolution would be too
slow (tests/test_gpu_properties.py, tests/test_gpu_wgrad_budget.py).

Weights are in the reference layout w[cs][cb][r][q] (Cs small-side channels, Cb big-side channels; nn.Conv2d(Cb -> Cs) weight,
nn.ConvTranspose2d(Cs -> Cb) weight), activations are logical NCHW tensors in any memory layout on any device; Hb = 2 * Hs:

  gather   small[b, cs, h, x] = sum_{cb, r, q} w[cs, cb, r, q] * big[b, cb, 2h - 2 + r, 2x - 2 + q]
  scatter  big[b, cb, y, x]   = sum_{cs, r, q : y = 2h - 2 + r, x = 2v - 2 + q} w[cs, cb, r, q] * small[b, cs, h, v]
  wgrad    dW[cs, cb, r, q]   = sum_{b, h, v} small[b, cs, h, v] * big[b, cb, 2h - 2 + r, 2v - 2 + q]

(out-of-range big pixels are zero).  Each function returns, per sampled element, r = sum a_i b_i and A = sum |a_i b_i| in float64:
A bounds what the rounding of the terms can do, so a kernel result `out` is checked as |out - r| <= tau * A.  Only the operand
elements a sample needs are gathered (advanced indexing on the device) before the conversion to float64; no library kernel is called.
"""
import torch

PAD, STRIDE, KS = 2, 2, 5


def gather_points(B, Hs, seed):
    """(b, h, x) samples of the gather output: rows and columns {0, 1, Hs/2, Hs-2, Hs-1}^2 (both borders and the middle) of images
    {0, B-1, one seeded random image}"""
    imgs = sorted({0, B - 1, int(torch.randint(0, B, (1,), generator=torch.Generator().manual_seed(seed)).item())})
    lines = sorted({0, 1, Hs // 2, Hs - 2, Hs - 1})
    return [(b, h, x) for b in imgs for h in lines for x in lines]


def scatter_points(B, Hb, seed):
    """(b, y, x) samples of the scatter output: rows and columns {0, 1, 2, 3, Hb/2, Hb/2+1, Hb-2, Hb-1}^2 -- both parities in both
    dimensions (all four phases of the stride-2 decomposition) at both borders and in the middle"""
    imgs = sorted({0, B - 1, int(torch.randint(0, B, (1,), generator=torch.Generator().manual_seed(seed)).item())})
    lines = sorted({0, 1, 2, 3, Hb // 2, Hb // 2 + 1, Hb - 2, Hb - 1})
    return [(b, y, x) for b in imgs for y in lines for x in lines]


def edge_channels(C):
    """channel indices at the edges of 64- and 128-wide tiles: {0, 63, 64, 127, 128, C-1}, those that exist"""
    return sorted({c for c in (0, 63, 64, 127, 128, C - 1) if 0 <= c < C})


def _idx(pts, device):
    t = torch.tensor(pts, dtype=torch.long, device=device)
    return t[:, 0], t[:, 1], t[:, 2]


def _contract(vals, w):
    """vals (n, 5, 5, C) float64 operand values per tap, w (C, D, 5, 5) -> r, A of shape (n, D)"""
    wd = w.detach().double()
    r = torch.einsum("nrqc,cdrq->nd", vals, wd)
    A = torch.einsum("nrqc,cdrq->nd", vals.abs(), wd.abs())
    return r, A


def gather_ref(big, w, pts):
    """r, A (len(pts), Cs) of the gather small[b, :, h, x] for (b, h, x) in pts; big (B, Cb, Hb, Wb), w (Cs, Cb, 5, 5)"""
    _, _, Hb, Wb = big.shape
    b, h, x = _idx(pts, big.device)
    tap = torch.arange(KS, device=big.device)
    yy = (STRIDE * h - PAD)[:, None] + tap[None, :]                      # (n, 5) big rows of tap r
    xx = (STRIDE * x - PAD)[:, None] + tap[None, :]                      # (n, 5) big columns of tap q
    ok = ((yy >= 0) & (yy < Hb))[:, :, None] & ((xx >= 0) & (xx < Wb))[:, None, :]
    yc, xc = yy.clamp(0, Hb - 1), xx.clamp(0, Wb - 1)
    vals = big[b[:, None, None], :, yc[:, :, None], xc[:, None, :]]      # (n, 5, 5, Cb), only the patches
    vals = vals.double() * ok[..., None]
    return _contract(vals, w.permute(1, 0, 2, 3))


def _scatter_src(y, n_small):
    """small row h feeding big row y through tap r (y = 2h - 2 + r), and whether that tap exists: (n, 5) each"""
    tap = torch.arange(KS, device=y.device)
    t = y[:, None] + PAD - tap[None, :]
    ok = (t % STRIDE == 0) & (t >= 0) & (t < STRIDE * n_small)
    return (t // STRIDE).clamp(0, n_small - 1), ok


def scatter_ref(small, w, pts):
    """r, A (len(pts), Cb) of the scatter big[b, :, y, x] for (b, y, x) in pts; small (B, Cs, Hs, Ws), w (Cs, Cb, 5, 5)"""
    _, _, Hs, Ws = small.shape
    b, y, x = _idx(pts, small.device)
    hs, okh = _scatter_src(y, Hs)
    vs, okv = _scatter_src(x, Ws)
    vals = small[b[:, None, None], :, hs[:, :, None], vs[:, None, :]]    # (n, 5, 5, Cs)
    vals = vals.double() * (okh[:, :, None] & okv[:, None, :])[..., None]
    return _contract(vals, w)


def scatter_terms(pts, Hs, Ws, Cs):
    """number of terms of each scatter sample (taps that exist x Cs): from 9 * Cs in the interior down to Cs at the far corner
    (Hb - 1, Wb - 1), which only tap (3, 3) reaches"""
    b, y, x = _idx(pts, "cpu")
    return _scatter_src(y, Hs)[1].sum(1) * _scatter_src(x, Ws)[1].sum(1) * Cs


def wgrad_ref(big, small, cs_list, cb_list):
    """r, A (len(cs_list), len(cb_list), 5, 5) of dW[cs, cb, :, :]: for each channel pair the full sum over all B * Hs * Ws pixels"""
    _, _, Hb, Wb = big.shape
    _, _, Hs, Ws = small.shape
    dev = big.device
    s = small[:, torch.tensor(cs_list, device=dev)].double()              # (B, ns, Hs, Ws): only the sampled channels
    g = big[:, torch.tensor(cb_list, device=dev)].double()                # (B, nb, Hb, Wb)
    g = torch.nn.functional.pad(g, (PAD, PAD, PAD, PAD))                  # zero border: padded row 2h + r = big row 2h - 2 + r
    r = torch.empty(len(cs_list), len(cb_list), KS, KS, dtype=torch.float64, device=dev)
    A = torch.empty_like(r)
    for i in range(KS):
        for j in range(KS):
            t = g[:, :, i:i + STRIDE * Hs:STRIDE, j:j + STRIDE * Ws:STRIDE]
            r[:, :, i, j] = torch.einsum("bshw,bchw->sc", s, t)
            A[:, :, i, j] = torch.einsum("bshw,bchw->sc", s.abs(), t.abs())
    return r, A


def take(out, pts):
    """kernel output out (B, C, H, W) at the sampled pixels, as (len(pts), C) float64"""
    b, h, x = _idx(pts, out.device)
    return out[b, :, h, x].double()


def worst(got, r, A):
    """max over the samples of |got - r| / A (A = 0, an all-zero sum, counts as 1) and the flat index of that sample"""
    e = (got.double() - r).abs() / torch.where(A > 0, A, torch.ones_like(A))
    i = int(e.flatten().argmax().item())
    return e.flatten()[i].item(), i
