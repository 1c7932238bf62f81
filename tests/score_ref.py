"""fp64 restatements, in plain torch, of the three scoring formulas of csrc/score.hip (include/vaeplay_hip.h).  Inputs of any
dtype are taken to fp64 first: an fp32 input is evaluated on exactly the values the kernel reads.  tests/test_infer_score_cpu.py
pins them against torch's own functions."""
import math

import torch


def bce_rows(p, t):
    """out[r] = sum_i -[t max(log p, -100) + (1 - t) max(log(1 - p), -100)] over everything but dimension 0"""
    p, t = p.double().reshape(p.shape[0], -1), t.double().reshape(t.shape[0], -1)
    lp, lq = torch.log(p).clamp_min(-100.0), torch.log(1.0 - p).clamp_min(-100.0)
    return -(t * lp + (1.0 - t) * lq).sum(1)


def latent_iw(mu, logvar, eps):
    """(z, kl, lr, scale): z = eps exp(logvar / 2) + mu; kl[b] = -1/2 sum_j (1 + logvar - mu^2 - exp(logvar));
    lr[b] = log p(z_b) - log q(z_b | x_b) = -1/2 sum_j z_j^2 + 1/2 sum_j (eps_j^2 + logvar_j); scale[b] = the sum of the absolute
    values of lr's terms, what a rounding error of the signed sum is relative to"""
    mu, logvar, eps = mu.double(), logvar.double(), eps.double()
    z = eps * torch.exp(0.5 * logvar) + mu
    kl = -0.5 * (1.0 + logvar - mu * mu - torch.exp(logvar)).sum(1)
    lr = -0.5 * (z * z).sum(1) + 0.5 * (eps * eps + logvar).sum(1)
    scale = 0.5 * (z * z + eps * eps + logvar.abs()).sum(1)
    return z, kl, lr, scale


def iw_bound(nbce, lr):
    """(logw, iwae): logw = -nbce + lr; iwae[b] = max_k logw + log(sum_k exp(logw - max)) - log K"""
    logw = -nbce.double() + lr.double()
    m = logw.max(1, keepdim=True).values
    return logw, m[:, 0] + torch.log(torch.exp(logw - m).sum(1)) - math.log(logw.shape[1])
