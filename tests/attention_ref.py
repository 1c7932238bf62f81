"""The fp64 statement of SelfAttentionBlock's core on (B, N, .) operands, y = gamma * softmax(q k^T) v + x, in plain torch with
autograd for the gradients; the input maker and the case table that tests/test_attention_cpu.py and tests/test_gpu_attention.py share."""
import torch

# (B, N, dq, C, scale, relu): N one below, at and above the kernels' 64-row tile (and 16, the MFMA tile); dq not a multiple of the
# MFMA depth 4; C across a channel chunk (64 / 128); the last case has |energy| up to ~230, so exp overflows fp32 without the max
CASES = [
    (2, 2, 1, 8, 1, 0),
    (2, 15, 4, 32, 1, 1),
    (3, 17, 5, 40, 1, 0),
    (1, 16, 4, 32, 1, 1),
    (2, 63, 3, 24, 1, 0),
    (2, 64, 8, 64, 1, 1),
    (2, 65, 12, 100, 1, 0),
    (2, 258, 32, 256, 1, 1),
    (1, 70, 90, 720, 1, 1),
    (2, 130, 8, 64, 4, 0),
]

Y_TOL = 2e-5          # tests/util.OP_RTOL
GRAD_TOL = 5e-5       # dq, dk, dv, dx: the bounds of tests/test_gpu_font.py::test_self_attention_block_matches_oracle
DGAMMA_ABS = 1e-5     # |dgamma - ref| <= DGAMMA_ABS * sum |g o|: a cancelling sum of B N C terms


def case_id(case):
    return "B{}_N{}_dq{}_C{}_s{}_r{}".format(*case)


def make(B, N, dq, C, scale=1, relu=0, seed=0, shift=0.0):
    """fp32 CPU operands: q, k = scale * randn (then ReLU if asked, then + shift), v, x, g = randn, gamma = 0.7."""
    gen = torch.Generator().manual_seed(1000 + seed)
    q = scale * torch.randn(B, N, dq, generator=gen)
    k = scale * torch.randn(B, N, dq, generator=gen)
    if relu:
        q, k = torch.relu(q), torch.relu(k)
    q, k = q + shift, k + shift
    v, x, g = (torch.randn(B, N, C, generator=gen) for _ in range(3))
    return {"q": q, "k": k, "v": v, "x": x, "g": g, "gamma": torch.full((1,), 0.7)}


def evaluate(inp, dtype=torch.float64):
    """y, o and the five gradients of sum(y * g), in ``dtype`` on the CPU, by autograd on the plain statement."""
    q, k, v, x, gamma = (inp[n].to(dtype).clone().requires_grad_(True) for n in ("q", "k", "v", "x", "gamma"))
    g = inp["g"].to(dtype)
    att = torch.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)
    o = torch.bmm(att, v)
    y = gamma * o + x
    y.backward(g)
    return {"y": y.detach(), "o": o.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad, "dx": x.grad, "dgamma": gamma.grad,
            "abs_go": (g * o.detach()).abs().sum()}


_REF = {}


def reference(case, seed=0, shift=0.0):
    """(inputs, fp64 results) of a table case, computed once per session and shared; callers must not modify either."""
    key = (tuple(case), seed, shift)
    if key not in _REF:
        inp = make(*case, seed=seed, shift=shift)
        _REF[key] = (inp, evaluate(inp))
    return _REF[key]
