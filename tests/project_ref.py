"""Restatements, in plain torch, of what latent projection computes (csrc/project.hip, infer.FusedVAEInference.project /
decode_grad).  The kernel formulas take inputs of any dtype to fp64 first: an fp32 input is evaluated on exactly the values the
kernel reads.  The decoder restatement is dtype-generic (fp64 or fp32, as tests/test_gpu_grad_accuracy.py evaluates its oracle) and
writes every ReLU as a multiplication by a 0/1 mask, so that the masks another implementation produced can be injected.
tests/test_infer_project_plan_cpu.py pins it to oracle.ref_cpu.decoder_forward(..., training=False) plus torch autograd."""
import torch
import torch.nn.functional as F


def bce_masked_rows(p, t, mask=None):
    """(out, dlogit): out[r] = sum_i mask * -[t max(log p, -100) + (1 - t) max(log(1 - p), -100)] over everything but dimension 0;
    dlogit = mask * (p - t), the gradient of out[r] with respect to the logits of p = sigmoid(logit); mask None: all ones"""
    p, t = p.double(), t.double()
    m = torch.ones_like(p) if mask is None else mask.double()
    lp, lq = torch.log(p).clamp_min(-100.0), torch.log(1.0 - p).clamp_min(-100.0)
    out = -(m * (t * lp + (1.0 - t) * lq)).reshape(p.shape[0], -1).sum(1)
    return out, m * (p - t)


def affine_relu_bwd(dy, u, scale):
    """dx[r][ch] = dy[r][ch] scale[ch] (u[r][ch] > 0): the backward through u = relu(scale c + shift) from its output, [R][C] views"""
    return dy.double() * scale.double() * (u > 0).double()


def latent_adam(z, g, m, v, step, lr, beta1, beta2, eps, prior_weight):
    """(z, m, v, prior) after torch.optim.Adam's step number ``step`` (1-based; no amsgrad, no weight decay) on the gradient
    g + prior_weight z; prior[r] = prior_weight / 2 |z_r|^2 of the z that came in"""
    z, g, m, v = z.double(), g.double(), m.double(), v.double()
    prior = 0.5 * prior_weight * (z * z).sum(1)
    gr = g + prior_weight * z
    m = m + (1.0 - beta1) * (gr - m)
    v = beta2 * v + (1.0 - beta2) * gr * gr
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    z = z - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    return z, m, v, prior


# ---- the eval-mode decoder with its ReLUs as masks ---------------------------------------------------------------------------------
def _bn_eval(p, prefix, x):
    from oracle import ref_cpu as O
    return F.batch_norm(x, p[prefix + ".running_mean"], p[prefix + ".running_var"], p[prefix + ".weight"], p[prefix + ".bias"], False,
                        O.BN_MOMENTUM, O.BN_EPS)


def decoder_masked(p, z, L, masks=None):
    """(x_tilde, masks used): models/networks.py:107-112 in eval mode, every ReLU a multiplication by a 0/1 mask -- masks=None
    derives them from the pre-activations (= F.relu), otherwise they are given, in layer order: the dense block (n, 64 size), then
    the L scatter blocks (n, C, H, W).  ``p``: the decoder's entries of the state dict ("decoder." prefix) in z's dtype."""
    dt, used = z.dtype, []

    def relu(t):
        m = (t > 0).to(dt) if masks is None else masks[len(used)].to(dt)
        used.append(m.detach())
        return t * m
    t = relu(_bn_eval(p, "decoder.fc.1", F.linear(z, p["decoder.fc.0.weight"]))).view(len(z), -1, 8, 8)
    for i in range(L):
        t = relu(_bn_eval(p, f"decoder.conv.{i}.bn",
                          F.conv_transpose2d(t, p[f"decoder.conv.{i}.conv.weight"], None, stride=2, padding=2, output_padding=1)))
    xt = torch.sigmoid(F.conv2d(t, p[f"decoder.conv.{L}.0.weight"], p[f"decoder.conv.{L}.0.bias"], stride=1, padding=2))
    return xt, used


def trained_params(C, S, z, B, seed=0):
    """An oracle state dict (fp32, host) with non-trivial eval state, made as tests/test_gpu_infer.py::_trained_vae makes its model:
    gamma ~ U(0.5, 1.5) and beta ~ N(0, 0.2) from a seeded generator, then three train-mode forwards of the CPU oracle on different
    seeded batches (momentum 0.9 moves the running statistics to the data's), so that a swapped or mis-indexed scale cannot pass
    and the decoder's output depends on z.  Returns (state dict, L)."""
    from oracle import ref_cpu as O
    L = O.iter_level_for(S)
    p = O.init_params(C, z, L, seed=seed)
    g = torch.Generator().manual_seed(100 + seed)
    for k, v in p.items():
        if k.endswith(("bn.weight", "fc.1.weight")):
            v.copy_(torch.empty(v.shape).uniform_(0.5, 1.5, generator=g))
        elif k.endswith(("bn.bias", "fc.1.bias")):
            v.copy_(torch.randn(v.shape, generator=g) * 0.2)
    with torch.no_grad():
        for k in range(3):
            xb = torch.rand((B, C, S, S), generator=torch.Generator().manual_seed(200 + k))
            eb = torch.randn((B, z), generator=torch.Generator().manual_seed(300 + k))
            O.vae_forward(p, xb, eb, L, training=True)
    return p, L


def z_star(n, z, seed=6):
    """the seeded latents whose decode is the target of the optimisation tests"""
    return torch.randn(n, z, generator=torch.Generator().manual_seed(seed))


def cast_params(state, dt):
    """the floating-point entries of a state dict on the host in dtype ``dt``"""
    return {k: (v.detach().cpu().to(dt) if v.dtype.is_floating_point else v.detach().cpu().clone()) for k, v in state.items()}


def decode_grad(p, z, x, L, mask=None, prior_weight=0.0, masks=None):
    """{x_tilde, bce (n,), loss (n,), dz (n, Z), masks} of the projection objective at z, in the dtype of ``p``:
    loss = sum over the image of mask * BCE(decode(z), x) + prior_weight / 2 |z|^2, dz = d loss / d z by autograd"""
    dt = p["decoder.fc.0.weight"].dtype
    z = z.detach().to(dt).clone().requires_grad_(True)
    x = x.to(dt)
    w = torch.ones_like(x) if mask is None else mask.to(dt)
    xt, used = decoder_masked(p, z, L, masks)
    bce = (w * F.binary_cross_entropy(xt, x, reduction="none")).reshape(len(x), -1).sum(1)
    loss = bce + 0.5 * prior_weight * (z * z).sum(1)
    (dz,) = torch.autograd.grad(loss.sum(), z)
    return {"x_tilde": xt.detach(), "bce": bce.detach(), "loss": loss.detach(), "dz": dz.detach(), "masks": used}


def project(p, x, L, z0, steps, lr, mask=None, prior_weight=1.0, betas=(0.9, 0.999), eps=1e-8):
    """the projection loop in the dtype of ``p``: (z, history (steps, n)) with history[i] the loss at the z iteration i started from"""
    dt = p["decoder.fc.0.weight"].dtype
    z = z0.to(dt).clone()
    m, v, hist = torch.zeros_like(z), torch.zeros_like(z), []
    for step in range(1, steps + 1):
        g = decode_grad(p, z, x, L, mask, 0.0)
        hist.append(g["bce"] + 0.5 * prior_weight * (z * z).sum(1))
        z, m, v, _ = latent_adam(z, g["dz"], m, v, step, lr, betas[0], betas[1], eps, prior_weight)
        z, m, v = z.to(dt), m.to(dt), v.to(dt)
    return z, torch.stack(hist) if hist else torch.zeros((0, len(x)), dtype=dt)
