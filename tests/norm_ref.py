"""What csrc/bn.hip computes, stated three times on the host (torch, CPU): reference() in float64, scales() -- the first-order fp32
error of a correct implementation, from the reference's own quantities -- and restate32(), the kernels' arithmetic in fp32 in the
kernels' order.  tests/test_gpu_norm_fp64.py asserts max |got - ref| / S <= K[output] for every output of every case of cases();
tests/test_norm_ref_cpu.py pins the reference to torch's autograd, the derivation of K to restate32, and shows by mutation that the
bound catches a dropped row, a skipped chunk, a wrong factor, a wrong image, a wrong sign and a dropped channel.

Everything is laid out [R][C] (rows = B*H*W or B, channels last) with an optional leading image axis for InstanceNorm; statistics
run over the rows."""
import torch

from tests import norm_cases as N
from tests.util import OP_RTOL

E = 2.0 ** -24                      # fp32 unit roundoff
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = N.ACTS
MASKED = (ACT_RELU, ACT_LRELU)      # activations whose derivative is a mask of the pre-activation's sign
MOMENTUM = 0.1
# The device's tanhf and __expf: tests/test_gpu_small_pointwise.py holds vp_act_fwd_f32 on tanh and sigmoid to OP_RTOL of max |y| = 1,
# so that is what the activation may add to y, in units of E (not measured on the kernels under test).
S_ACT = OP_RTOL / E

# One constant per output kind: 4 x the worst ratio of restate32 against reference over cases(), measured on the CPU (the figure in
# the comment; tests/test_norm_ref_cpu.py::test_restatement_is_within_a_quarter_of_K asserts ratio <= K / 4).  The factor 4 is for the
# kernels' different but equally valid summation order and fma contraction.  Fixed before any GPU run.
K = {
    "mean": 15.0,           # 3.55  BatchNorm 32 x 1024, no activation
    "rstd": 12.5,           # 3.03  BatchNorm 32 x 1024
    "running_mean": 9.6,    # 2.35  BatchNorm 4 x 32768
    "running_var": 9.4,     # 2.29  BatchNorm 63 x 60
    "y": 40.0,              # 9.91  InstanceNorm 3 x 65 x 68, ReLU
    "dbeta": 3.2,           # 0.770 BatchNorm 4 x 32768
    "dgamma": 3.8,          # 0.937 BatchNorm 4 x 32768, leaky ReLU
    "dx": 5.4,              # 1.33  BatchNorm 32 x 1024
}


def f32(v):
    """a Python float as the C ABI passes it (a float argument)"""
    return float(torch.tensor(v, dtype=torch.float32))


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------
def _act(u, act, slope):
    if act == ACT_RELU:
        return torch.where(u > 0, u, torch.zeros_like(u))
    if act == ACT_LRELU:
        return torch.where(u > 0, u, u * slope)
    if act == ACT_TANH:
        return torch.tanh(u)
    if act == ACT_SIGMOID:
        return 1 / (1 + torch.exp(-u))
    return u


def _dact(u, act, slope, mask=None):
    one = torch.ones_like(u)
    if act in MASKED:
        return torch.where((u > 0) if mask is None else mask, one, one * (0.0 if act == ACT_RELU else slope))
    if act == ACT_TANH:
        return 1 - torch.tanh(u) ** 2
    if act == ACT_SIGMOID:
        s = 1 / (1 + torch.exp(-u))
        return s * (1 - s)
    return one


def reference(x, dy, gamma, beta, act, slope, eps, momentum, batch_stats, mask=None, mean=None, rstd=None, rm=None, rv=None):
    """-> dict of float64 tensors: mean, rstd [..][C]; y, dx [..][R][C]; dgamma, dbeta [..][C]; running_mean, running_var where rm,
    rv are given; and the quantities scales() needs (x0, var, xhat, u, g, dy, gamma, R, batch_stats, act, given)."""
    x, dy = x.double(), dy.double()
    R, C = x.shape[-2:]
    ga = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    be = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    bmean = x.mean(-2)
    bvar = ((x - bmean.unsqueeze(-2)) ** 2).mean(-2)                       # two passes, biased
    given = mean is not None
    mu = mean.double() if given else bmean
    rs = rstd.double() if given else 1 / torch.sqrt(bvar + eps)
    xhat = (x - mu.unsqueeze(-2)) * rs.unsqueeze(-2)
    u = ga * xhat + be
    y = _act(u, act, slope)
    g = dy * _dact(u, act, slope, mask)
    dbeta, dgamma = g.sum(-2), (g * xhat).sum(-2)
    k = (dbeta.unsqueeze(-2) + xhat * dgamma.unsqueeze(-2)) / R if batch_stats else 0.0
    dx = ga * rs.unsqueeze(-2) * (g - k)
    out = dict(mean=mu, rstd=rs, y=y, dx=dx, dgamma=dgamma, dbeta=dbeta, x0=x[..., 0, :], var=bvar, xhat=xhat, u=u, g=g, dy=dy, gamma=ga,
               R=R, batch_stats=batch_stats, act=act, given=given, momentum=momentum)
    if rm is not None:
        out["running_mean"] = (1 - momentum) * rm.double() + momentum * bmean
    if rv is not None:
        out["running_var"] = (1 - momentum) * rv.double() + momentum * (bvar * R / (R - 1) if R > 1 else bvar)   # R = 1: as bn_finalize
    return out


def scales(ref):
    """-> dict, for every output of reference(), of S (same shape): the first-order fp32 error of a correct implementation.
    With e = 2^-24, kappa = |mean| rstd (rounding the mean to fp32 moves xhat by kappa e) and p = ((x[row 0] - mean) rstd)^2 (the
    cancellation of the row-0 pivot in bn_finalize).  Given statistics (eval mode) are exact fp32 inputs: their own error, and the
    kappa term, are then 0."""
    e, R, act = E, ref["R"], ref["act"]
    mean, rstd, xhat, ga, g, dy = ref["mean"], ref["rstd"], ref["xhat"], ref["gamma"].abs(), ref["g"], ref["dy"].abs()
    up = lambda t: t.unsqueeze(-2)
    if ref["given"]:
        S_mean, S_rstd, kappa = torch.zeros_like(mean), torch.zeros_like(rstd), torch.zeros_like(mean)
    else:
        p = ((ref["x0"] - mean) * rstd) ** 2
        S_mean = e * (mean.abs() + 1 / rstd)
        S_rstd = e * rstd * (1 + p)
        kappa = mean.abs() * rstd
    S_xhat = e * (up(kappa) + 2 * xhat.abs()) + xhat.abs() * up(S_rstd / rstd)
    s_act = S_ACT if act in (ACT_TANH, ACT_SIGMOID) else 0.0
    c_act = 1.0 if act in (ACT_TANH, ACT_SIGMOID) else 0.0
    S_y = ga * S_xhat + e * (ref["y"].abs() + s_act)
    S_g = dy * (2 * e + c_act * ga * S_xhat)
    S_dbeta = S_g.sum(-2) + e * g.abs().sum(-2)
    S_dgamma = (S_g * xhat.abs() + g.abs() * S_xhat).sum(-2) + e * (g * xhat).abs().sum(-2)
    bs = 1.0 if ref["batch_stats"] else 0.0
    S_dx = (ga * up(rstd) * (S_g + bs * (up(S_dbeta) + xhat.abs() * up(S_dgamma)) / R + bs * up((ref["dgamma"] / R).abs()) * S_xhat)
            + ref["dx"].abs() * (2 * e + up(S_rstd / rstd)))
    S = dict(mean=S_mean, rstd=S_rstd, y=S_y, dbeta=S_dbeta, dgamma=S_dgamma, dx=S_dx)
    m = ref["momentum"]
    if "running_mean" in ref:
        S["running_mean"] = m * S_mean + e * ref["running_mean"].abs()
    if "running_var" in ref:
        S["running_var"] = m * 2 * ref["var"] * (S_rstd / rstd) * (R / (R - 1) if R > 1 else 1.0) + e * ref["running_var"].abs()
    return S


def ratios(got, ref, S):
    """-> {output: max |got - ref| / S} over the outputs of got that have a scale (0 / 0 counts as 0)"""
    out = {}
    for k, t in got.items():
        if k not in S or t is None:
            continue
        d = (t.detach().double().cpu().reshape(ref[k].shape) - ref[k]).abs()
        assert torch.isfinite(d).all(), f"{k}: not finite"
        out[k] = torch.where(d == 0, torch.zeros_like(d), d / S[k]).max().item()
    return out


def mask_disagreements(y_got, ref, S):
    """number of elements with |u| > K[y] S_y (S_y is the error scale of u for ReLU and leaky ReLU) at which y_got > 0 differs from
    the fp64 u > 0"""
    u = ref["u"]
    sure = u.abs() > K["y"] * S["y"]
    return int((((y_got.detach().cpu().reshape(u.shape) > 0) != (u > 0)) & sure).sum())


# ---- the kernels' arithmetic in fp32, in the kernels' order ---------------------------------------------------------------------------
def bn_grid(R, C):
    """bn.hip's bn_grid -> chunks_r, rows_per_chunk"""
    want = max(1, 1024 // ((C + 63) // 64))
    chunks = min(want, max(1, (R + 63) // 64))
    rpc = (R + chunks - 1) // chunks
    return (R + rpc - 1) // rpc, rpc


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64"""
    return (a.double() * b.double() + c.double()).float()


def _walk(R, C, mutate):
    """rows [chunk][trip][row lane] that thread row lane ty of a chunk visits, trip after trip (walk_rows), and which of them exist"""
    chunks, rpc = bn_grid(R, C)
    k = torch.arange(chunks).view(-1, 1, 1)
    t = torch.arange((rpc + 15) // 16).view(1, -1, 1)
    ty = torch.arange(16).view(1, 1, -1)
    local = t * 16 + ty + 0 * k
    rows = k * rpc + local
    valid = (local < rpc) & (rows < R)
    if mutate == "drop_row":                  # the last row of one chunk is never visited
        valid[chunks // 2, (rpc - 1) // 16, (rpc - 1) % 16] = False
    return rows.clamp(max=R - 1), valid


def _chunk_sums(a, b, R, C, mutate):
    """(sum a, sum a * b) over the rows as bn_partial_kernel + bn_final_reduce take them: per row lane in row order (sum_pair), the 16
    lanes in lane order (block_colsum), the chunks in fp64.  a, b: fp32 [B][R][C] -> fp64 [B][C] each."""
    rows, valid = _walk(R, C, mutate)
    v = valid.unsqueeze(0).unsqueeze(-1)
    A = torch.where(v, a[:, rows], torch.zeros((), dtype=a.dtype))      # [B][chunk][trip][lane][C]
    Bv = torch.where(v, b[:, rows], torch.zeros((), dtype=b.dtype))
    s = torch.zeros_like(A[:, :, 0])
    q = torch.zeros_like(s)
    for t in range(A.shape[2]):
        s = s + A[:, :, t]
        q = _fma(A[:, :, t], Bv[:, :, t], q)
    ts, tq = torch.zeros_like(s[:, :, 0]), torch.zeros_like(s[:, :, 0])
    for lane in range(16):
        ts = ts + s[:, :, lane]
        tq = tq + q[:, :, lane]
    keep = torch.ones(ts.shape[1], dtype=torch.bool)
    if mutate == "skip_chunk":                # the finaliser's second chain (chunk k + 64 of every 128) is never added
        keep = torch.arange(ts.shape[1]) % 128 < 64
    return ts[:, keep].double().sum(1), tq[:, keep].double().sum(1)


def _act32(u, act, slope):
    if act == ACT_RELU:
        return torch.where(u > 0, u, torch.zeros_like(u))
    if act == ACT_LRELU:
        return torch.where(u > 0, u, u * slope)
    if act == ACT_TANH:
        return torch.tanh(u)
    if act == ACT_SIGMOID:
        return 1 / (1 + torch.exp(-u))
    return u


def _dact32(u, act, slope):
    one = torch.ones_like(u)
    if act == ACT_RELU:
        return torch.where(u > 0, one, torch.zeros_like(u))
    if act == ACT_LRELU:
        return torch.where(u > 0, one, one * slope)
    if act == ACT_TANH:
        t = torch.tanh(u)
        return 1 - t * t
    if act == ACT_SIGMOID:
        s = 1 / (1 + torch.exp(-u))
        return s * (1 - s)
    return one


def restate32(x, dy, gamma, beta, act, slope, eps, momentum, batch_stats, mean=None, rstd=None, rm=None, rv=None, mutate=None):
    """bn.hip in fp32 torch -> dict of fp32 tensors (mean, rstd, y, u, dx, dgamma, dbeta, running_mean, running_var), shaped as
    reference()'s.  Not bit-exact to the GPU (torch's tanh and exp, no contraction): it fixes K from something that is not the code
    under test.  mutate plants one fault (tests/test_norm_ref_cpu.py)."""
    f = torch.float32
    batched = x.dim() == 3
    x, dy = (t.to(f) if batched else t.to(f).unsqueeze(0) for t in (x, dy))
    B, R, C = x.shape
    slope, mom = torch.tensor(slope, dtype=f), torch.tensor(momentum, dtype=f)
    ga = torch.ones(C, dtype=f) if gamma is None else gamma.to(f)
    be = torch.zeros(C, dtype=f) if beta is None else beta.to(f)
    out = {}
    if mean is None:
        pivot = x[:, 0, :].clone()                                           # the channel's value in row 0 of its image
        if mutate == "pivot_image":
            pivot[2] = pivot[0]
        d = x - pivot.unsqueeze(1)
        s, q = _chunk_sums(d, d, R, C, mutate)
        ms = s / R                                                           # bn_finalize, in fp64
        var = (q / R - ms * ms).clamp(min=0.0)
        m = pivot.double() + ms
        mu, rs = m.float(), (1.0 / torch.sqrt(var + float(eps))).float()
        one = torch.tensor(1.0, dtype=f)
        if rm is not None:
            out["running_mean"] = ((one - mom) * rm.to(f) + mom * m.float()[0])
        if rv is not None:
            unb = var * R / ((R if mutate == "rv_R" else R - 1)) if R > 1 else var
            out["running_var"] = ((one - mom) * rv.to(f) + mom * unb.float()[0])
    else:
        mu, rs = (t.to(f) if batched else t.to(f).unsqueeze(0) for t in (mean, rstd))
    mu_, rs_ = mu.unsqueeze(1), rs.unsqueeze(1)
    xh = (x - mu_) * rs_
    u = _fma(ga.expand_as(xh), xh, be.expand_as(xh))                         # bn_pre, the same in forward and backward
    y = _act32(u, act, slope)
    g = dy * _dact32(u, act, slope)                                          # bn_g
    sg, sgx = _chunk_sums(g, xh, R, C, mutate)
    sum_g, sum_gx = sg.float(), sgx.float()
    invR = (torch.tensor(1.0, dtype=f) / torch.tensor(float(R), dtype=f)) if batch_stats else torch.tensor(0.0, dtype=f)
    if C % 4 == 0:                                                           # bn_dx of the tiled and the small kernels
        k0, k1 = (sum_g * invR).unsqueeze(1), (sum_gx * invR).unsqueeze(1)
        if mutate == "k1_sign":
            k1 = -k1
        dx = (ga * rs_) * (g - _fma(xh, k1.expand_as(xh), k0.expand_as(xh)))
    else:                                                                    # bn_act_bwd_kernel, in its own order
        dx = (ga * rs_) * (g - (sum_g.unsqueeze(1) + xh * sum_gx.unsqueeze(1)) * invR)
    out.update(mean=mu, rstd=rs, y=y, u=u, dx=dx, dgamma=sum_gx, dbeta=sum_g)
    if mutate == "drop_channel":              # the last channel is never computed
        for k in ("mean", "rstd", "y", "dx", "dgamma", "dbeta", "running_mean", "running_var"):
            if k in out:
                out[k] = out[k].clone()
                out[k][..., C - 1] = 0.0
    if not batched:
        out = {k: (t[0] if k not in ("running_mean", "running_var") else t) for k, t in out.items()}
    return out


# ---- the cases of tests/test_gpu_norm_fp64.py, and the same cases through restate32 ----------------------------------------------------
BWD_SHAPES = [(65, 68), (70, 3), (200, 12)]
BWD_VARIANTS = [("eval", 0), ("null_affine", 0), ("null_affine", 1), ("no_affine_grads", 0), ("no_affine_grads", 1)]
FMT_SHAPES = [(65, 68), (8300, 8)]


def inorm_act(B, R, C):
    return N.ACTS[(B + R + C) % len(N.ACTS)]       # as tests/test_gpu_norm_edges.py cycles them


def cases():
    """every case as a dict: kind bn | bwd | inorm, its shape and activation"""
    out = [dict(kind="bn", B=1, R=R, C=C, act=a) for R, C in N.BN_SHAPES for a in N.ACTS]
    out += [dict(kind="bwd", B=1, R=R, C=C, act=a, variant=v, batch_stats=bs) for R, C in BWD_SHAPES for v, bs in BWD_VARIANTS for a in N.ACTS]
    out += [dict(kind="inorm", B=B, R=R, C=C, act=inorm_act(B, R, C), offset=0.0) for B, R, C in N.BATCHED]
    out += [dict(kind="inorm", B=B, R=R, C=C, act=a, offset=N.OFFSET) for B, R, C in N.OFFSET_BATCHED for a in N.ACTS]
    return out


def case_id(c):
    s = f"{c['kind']}-{c['B']}x{c['R']}x{c['C']}-act{c['act']}"
    if c["kind"] == "bwd":
        s += f"-{c['variant']}-bs{c['batch_stats']}"
    if c.get("offset"):
        s += "-offset"
    return s


def given_stats(x):
    """eval-mode statistics [C] for x [R][C]: the batch's, perturbed (a running average never equals the batch), as fp32"""
    g = torch.Generator().manual_seed(x.shape[0] * 131 + x.shape[1])
    x = x.double().cpu()
    mean = x.mean(0) + 0.5 * torch.randn(x.shape[1], generator=g, dtype=torch.float64)
    rstd = (0.8 + 0.4 * torch.rand(x.shape[1], generator=g, dtype=torch.float64)) / torch.sqrt(x.var(0, unbiased=False) + N.EPS)
    return mean.float(), rstd.float()


def running_init(C):
    """the running statistics norm_cases.bn_stats starts from"""
    return torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C)


def case_args(c, x, dy, gamma, beta):
    """the arguments of reference() / restate32() after (x, dy) for a case: CPU tensors in, kwargs out"""
    kw = dict(gamma=gamma, beta=beta, act=c["act"], slope=f32(N.SLOPE), eps=f32(N.EPS), momentum=f32(MOMENTUM), batch_stats=1)
    if c["kind"] == "bn":
        kw["rm"], kw["rv"] = running_init(c["C"])
    elif c["kind"] == "inorm":
        kw.update(gamma=None, beta=None, momentum=0.0)
    else:
        kw["batch_stats"] = c["batch_stats"]
        if c["variant"] == "null_affine":
            kw.update(gamma=None, beta=None)
        if c["batch_stats"] == 0:
            kw["mean"], kw["rstd"] = given_stats(x)
    return kw


def restate_case(c, mutate=None):
    """a case on the CPU -> (restate32's outputs, the reference with the restatement's own mask, its scales)"""
    x, dy, gamma, beta, _ = N.inputs(c["B"], c["R"], c["C"], offset=c.get("offset", 0.0), device="cpu")
    if c["kind"] != "inorm":
        x, dy = x[0], dy[0]
    kw = case_args(c, x, dy, gamma, beta)
    got = restate32(x, dy, mutate=mutate, **kw)
    ref = reference(x, dy, mask=(got["y"] > 0) if c["act"] in MASKED else None, **kw)
    return got, ref, scales(ref)
