"""What tests/test_gpu_small_edges.py and tools/ab_small_bits.py share: the smallest shapes at which the paths of the small kernels
change (csrc/elementwise.hip, optim.hip, score.hip, project.hip), and every entry point of those files called on guarded buffers
(tests/guarded.py) with an exact-size workspace.  A case is (function, arguments, is-a-reduction); the function takes a
norm_cases.Lib and returns {name: tensor} of every output, workspace query and updated state.  Inputs are drawn from a seed the
arguments fix, so two calls of a case see the same inputs.

Flat kernels walk 256-thread workgroups with a capped grid; the large sizes are the ones tests/test_gpu_small_*.py and
test_gpu_flat_optim.py use to reach the next trip of each capped loop.  BCE inputs hold p = 0 and p = 1 exactly (the -100 clamp)."""
import torch

from tests.guarded import Guards, gen

FLAT_N = [1, 3, 4, 5, 1027]
FLAT_BIG = 2 * 524288 + 77                  # grid_for's default cap: 2048 blocks = 524,288 items
REDUCE_BIG = 2 * 1048576 + 4000 + 3         # reduce_blocks' 1024 blocks of quads; RMSprop's and affine_relu_bwd's 4096 blocks
QUAD_BIG = 2 * 2097152 + 7                  # bce_sigmoid_bwd: 2048 blocks of quads
ADAM_N = [1, 7, 1027, 4 * (16384 * 256 + 1000) + 3]      # the last: the two-quad loop, the single quad and the tail all run
ADAM_OUTER = [(1, 4, 4), (3, 8, 1024), (5, 12, 1028)]
LR, B1, B2, EPS, ALPHA = 1e-3, 0.9, 0.999, 1e-8, 0.99


def _env():
    from vae_play_amd import ops
    return ops._pv, ops._stream()


def _r(seed, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=gen(seed)) * scale + shift).cuda()


def _u(seed, *shape):
    return torch.rand(*shape, generator=gen(seed)).cuda()


def probs(seed, *shape):
    """uniform (0, 1) with an exact 0 first and, from two elements on, an exact 1 in the middle"""
    p = torch.rand(*shape, generator=gen(seed))
    f = p.view(-1)
    f[0] = 0.0
    if f.numel() > 1:
        f[f.numel() // 2] = 1.0
    return p.cuda()


def flat_case(L, n):
    """the pointwise kernels over n elements"""
    P, st = _env()
    G, o = Guards(), {}
    a, b, g = _r(n, n), _r(n + 1, n), _r(n + 2, n)
    p, t = probs(n + 3, n), _u(n + 4, n)
    g1 = _r(n + 5, 1)
    o["add"] = G.out("add", n)
    L.call("vp_add_f32", P(a), P(b), P(o["add"]), n, st)
    o["half_sqdiff"] = G.out("hs", n)
    L.call("vp_half_sqdiff_f32", P(a), P(b), P(o["half_sqdiff"]), n, st)
    for per_row, gg in ((0, g), (1, g1)):
        da, db = G.out("da", n), G.out("db", n)
        L.call("vp_half_sqdiff_bwd_f32", P(a), P(b), P(gg), P(da), P(db), 1, n, per_row, st)
        o[f"half_sqdiff_bwd {per_row} da"], o[f"half_sqdiff_bwd {per_row} db"] = da, db
    o["bce_bwd"] = G.out("dp", n)
    L.call("vp_bce_bwd_f32", P(p), P(t), P(g1), 0.5, P(o["bce_bwd"]), n, st)
    o["bce_sigmoid_bwd"] = G.out("dl", n)
    L.call("vp_bce_sigmoid_bwd_f32", P(p), P(t), 0.25, P(o["bce_sigmoid_bwd"]), n, st)
    da, db = G.out("l1 da", n), G.out("l1 db", n)
    L.call("vp_l1_mean_bwd_f32", P(a), P(b), P(g1), P(da), P(db), n, st)
    o["l1_bwd da"], o["l1_bwd db"] = da, db
    C = 4 if n % 4 == 0 else 1                  # affine_relu_bwd: the 16-byte kernel and the element-by-element one
    scale = _r(n + 6, C)
    dx, dxs = G.out("ar dx", n), G.planes("ar dxs", n)
    L.call("vp_affine_relu_bwd_f32", P(g), P(a), None, P(scale), P(dx), P(dxs), n // C, C, st)
    o["affine_relu_bwd dx"], o["affine_relu_bwd planes"] = dx, dxs
    G.check()
    return o


def channels_case(L, npix):
    """the pointwise kernels that walk pixels x channels"""
    P, st = _env()
    G, o = Guards(), {}
    p, t = probs(npix, npix, 3), _u(npix + 1, npix, 3)
    dl, dls = G.out("dl", npix * 3), G.planes("dls", npix * 8)
    L.call("vp_bce_sigmoid_bwd_pad_split_f32", P(p), P(t), 0.25, P(dl), P(dls), npix, 3, 8, st)
    o["pad_split dl"], o["pad_split planes"] = dl, dls
    x = _r(npix + 2, npix, 5)
    o["slice"] = G.out("slice", npix * 3)
    L.call("vp_slice_channels_f32", P(x), P(o["slice"]), npix, 5, 3, st)
    for norm in (0, 1):
        o[f"add_coords {norm}"] = G.out("coords", npix * 7)
        L.call("vp_add_coords_f32", P(x), P(o[f"add_coords {norm}"]), 1, npix, 1, 5, norm, st)
    G.check()
    return o


def reduce_case(L, n):
    """the two-stage scalar reductions"""
    P, st = _env()
    G, o = Guards(), {}
    p, t, x = probs(n, n), _u(n + 1, n), _r(n + 2, n)
    kl = _r(n + 3, 5, shift=3.0)
    nb = L.h.vp_reduce_workspace_bytes(n)
    o["ws_bytes"] = torch.tensor([nb])
    ws, _ = G.ws("ws", nb)
    o["bce_sum"] = G.out("bce", 1)
    L.call("vp_bce_sum_f32", P(p), P(t), n, P(o["bce_sum"]), P(ws), nb, st)
    ws, _ = G.ws("ws", nb)
    recon, kls, loss = G.out("recon", 1), G.out("kl_sum", 1), G.out("loss", 1)
    L.call("vp_vae_loss_f32", P(p), P(t), n, P(kl), 5, P(recon), P(kls), P(loss), 1.0 / 5, P(ws), nb, st)
    o["vae recon"], o["vae kl_sum"], o["vae loss"] = recon, kls, loss
    ws, _ = G.ws("ws", nb)
    o["sum"] = G.out("sum", 1)
    L.call("vp_sum_f32", P(x), n, P(o["sum"]), P(ws), nb, st)
    ws, _ = G.ws("ws", 2 * nb)
    o["l1_mean"] = G.out("l1", 1)
    L.call("vp_l1_mean_f32", P(x), P(t), n, P(o["l1_mean"]), P(ws), 2 * nb, st)
    G.check()
    return o


def adam_case(L, n, step, grad_scale):
    P, st = _env()
    G = Guards()
    p, m = G.state("p", _r(n, n).cpu()), G.state("m", _r(n + 1, n, scale=0.1).cpu())
    v = G.state("v", (_u(n + 2, n) * 0.5 + 1e-3).cpu())
    g = _r(n + 3, n, scale=2.0)
    L.call("vp_adam_f32", P(p), P(g), P(m), P(v), n, LR, B1, B2, EPS, step, grad_scale, st)
    G.check()
    return {"p": p, "m": m, "v": v}


def rmsprop_case(L, n):
    P, st = _env()
    G = Guards()
    p, sq = G.state("p", _r(n, n).cpu()), G.state("sq", (_u(n + 2, n) * 0.5 + 1e-3).cpu())
    g = _r(n + 3, n, scale=2.0)
    L.call("vp_rmsprop_f32", P(p), P(g), P(sq), n, LR, ALPHA, EPS, 0.25, st)
    G.check()
    return {"p": p, "sq": sq}


def adam_outer_inputs(K, R, Cn):
    """A [K][R], B [K][Cn], and p, m, v [R][Cn] on the host"""
    s = K * 7919 + R * 131 + Cn
    A, Bm = torch.randn(K, R, generator=gen(s)), torch.randn(K, Cn, generator=gen(s + 1))
    p, m = torch.randn(R, Cn, generator=gen(s + 2)), torch.randn(R, Cn, generator=gen(s + 3)) * 0.1
    v = torch.rand(R, Cn, generator=gen(s + 4)) * 0.5 + 1e-3
    return A, Bm, p, m, v


def adam_outer_case(L, K, R, Cn, step=3, grad_scale=0.25):
    P, st = _env()
    G = Guards()
    A, Bm, p0, m0, v0 = adam_outer_inputs(K, R, Cn)
    p, m, v = G.state("p", p0), G.state("m", m0), G.state("v", v0)
    A, Bm = A.cuda(), Bm.cuda()
    L.call("vp_adam_outer_f32", P(p), P(m), P(v), P(A), P(Bm), K, R, Cn, LR, B1, B2, EPS, step, grad_scale, st)
    G.check()
    return {"p": p, "m": m, "v": v}


def latent_adam_case(L, rows, Z, prior_weight):
    """two steps from a counter of 2 (steps 3 and 4), then the prior-only call on the result"""
    P, st = _env()
    G = Guards()
    s = rows * 1000 + Z
    z, m = G.state("z", _r(s, rows, Z).cpu()), G.state("m", _r(s + 1, rows, Z, scale=0.1).cpu())
    v = G.state("v", (_u(s + 2, rows, Z) * 0.5 + 1e-3).cpu())
    count = G.state("count", torch.tensor([2], dtype=torch.int32).view(torch.float32))
    o = {}
    for k in range(2):
        g = _r(s + 3 + k, rows, Z, scale=2.0)
        prior = G.out("prior", rows)
        L.call("vp_latent_adam_f32", P(z), P(g), P(m), P(v), P(count), rows, Z, LR, B1, B2, EPS, prior_weight, P(prior), st)
        o.update({f"step {k} z": z.clone(), f"step {k} m": m.clone(), f"step {k} v": v.clone(), f"step {k} prior": prior})
    o["count"] = count.view(torch.int32).clone()
    o["prior alone"] = G.out("prior", rows)
    L.call("vp_latent_adam_f32", P(z), None, None, None, None, rows, Z, LR, B1, B2, EPS, prior_weight, P(o["prior alone"]), st)
    G.check()
    return o


def be_case(L, B, n):
    """BE loss (logits) and dice loss (probabilities), forward and backward"""
    P, st = _env()
    G, o = Guards(), {}
    s = B * 100003 + n
    x, pr, t, g1 = _r(s, B, n, scale=3.0), _u(s + 1, B, n), (_u(s + 2, B, n) > 0.5).float(), _r(s + 3, 1)
    nb = L.h.vp_be_loss_workspace_bytes(B, n)
    o["ws_bytes"] = torch.tensor([nb])
    for name, src, extra in (("be", x, (0.7, 1.0)), ("dice", pr, (1.0,))):
        ws, _ = G.ws("ws", nb)
        loss, sums, dx = G.out("loss", 1), G.out("sums", B, 4), G.out("dx", B, n)
        L.call(f"vp_{name}_loss_fwd_f32", P(src), P(t), P(loss), P(sums), B, n, *extra, P(ws), nb, st)
        L.call(f"vp_{name}_loss_bwd_f32", P(src), P(t), P(sums), P(g1), P(dx), B, n, *extra, st)
        o.update({f"{name} loss": loss, f"{name} sums": sums, f"{name} dx": dx})
    G.check()
    return o


def rowsum_case(L, n, R=3):
    P, st = _env()
    G = Guards()
    a, b = _r(n, R, n), _r(n + 1, R, n)
    out = G.out("rowsum", R)
    L.call("vp_half_sqdiff_rowsum_f32", P(a), P(b), P(out), R, n, st)
    G.check()
    return {"rowsum": out}


def gan_head_case(L, B):
    P, st = _env()
    G = Guards()
    logit = _r(B, 3 * B, scale=6.0)
    logit[0] = 40.0                 # saturated: y rounds to 1
    p, sums, dl = G.out("p", 3 * B), G.out("sums", 3), G.out("dlogit", 3 * B)
    L.call("vp_gan_head_f32", P(logit), B, 0.3, P(p), P(sums), P(dl), st)
    G.check()
    return {"p": p, "sums": sums, "dlogit": dl}


def smooth_l1_case(L, B, n1, n2):
    P, st = _env()
    G = Guards()
    s = B * 1009 + n1 * 31 + n2
    t, a = _r(s, B, n1 + n2, scale=2.0), _r(s + 1, B, n1)
    b = _r(s + 2, B, n2) if n2 else None
    loss, da = G.out("loss", 1), G.out("da", B, n1)
    db = G.out("db", B, n2) if n2 else None
    L.call("vp_smooth_l1_cat_f32", P(t), P(a), P(b), B, n1, n2, 0.5, P(loss), P(da), P(db), st)
    G.check()
    return {"loss": loss, "da": da, "db": db}


def softmax_case(L, R, n):
    P, st = _env()
    G = Guards()
    x, dy = _r(R * 1000 + n, R, n, scale=3.0), _r(R * 1000 + n + 1, R, n)
    y, dx = G.out("y", R, n), G.out("dx", R, n)
    L.call("vp_softmax_rows_fwd_f32", P(x), P(y), R, n, st)
    L.call("vp_softmax_rows_bwd_f32", P(y), P(dy), P(dx), R, n, st)
    G.check()
    return {"y": y, "dx": dx}


def cross_entropy_case(L, R, n):
    P, st = _env()
    G = Guards()
    x, g1 = _r(R * 1000 + n, R, n, scale=3.0), _r(R + n, 1)
    labels = torch.randint(0, n, (R,), generator=gen(R + 7 * n)).cuda()
    loss, prob, dx = G.out("loss", 1), G.out("prob", R, n), G.out("dx", R, n)
    L.call("vp_cross_entropy_fwd_f32", P(x), P(labels), P(loss), P(prob), R, n, st)
    L.call("vp_cross_entropy_bwd_f32", P(prob), P(labels), P(g1), P(dx), R, n, st)
    G.check()
    return {"loss": loss, "prob": prob, "dx": dx}


def latent_case(L, B, Z):
    """latent forward and backward, the importance-weighted forward and the bound over the same [B][Z] values"""
    P, st = _env()
    G = Guards()
    s = B * 1000003 + Z
    mu, lv, eps, dz, gkl = _r(s, B, Z), _r(s + 1, B, Z, scale=0.5), _r(s + 2, B, Z), _r(s + 3, B, Z), _r(s + 4, B)
    z, kl, dmu, dlv = G.out("z", B, Z), G.out("kl", B), G.out("dmu", B, Z), G.out("dlv", B, Z)
    L.call("vp_latent_fwd_f32", P(mu), P(lv), P(eps), P(z), P(kl), B, Z, st)
    L.call("vp_latent_bwd_f32", P(mu), P(lv), P(eps), P(dz), P(gkl), 0.125, P(dmu), P(dlv), B, Z, st)
    z2, kl2, lr = G.out("iw z", B, Z), G.out("iw kl", B), G.out("iw lr", B)
    L.call("vp_latent_iw_fwd_f32", P(mu), P(lv), P(eps), P(z2), P(kl2), P(lr), B, Z, st)
    logw, iwae = G.out("logw", B, Z), G.out("iwae", B)
    L.call("vp_iw_bound_f32", P(mu), P(dz), B, Z, P(logw), P(iwae), st)
    G.check()
    return {"z": z, "kl": kl, "dmu": dmu, "dlv": dlv, "iw z": z2, "iw kl": kl2, "iw lr": lr, "logw": logw, "iwae": iwae}


def avgpool_case(L, C, HW, B=2):
    P, st = _env()
    G = Guards()
    x, dy = _r(C * 100 + HW, B, HW, C), _r(C * 100 + HW + 1, B, C)
    out, dx = G.out("out", B, C), G.out("dx", B, HW, C)
    L.call("vp_global_avgpool_fwd_f32", P(x), P(out), B, HW, C, st)
    L.call("vp_global_avgpool_bwd_f32", P(dy), P(dx), B, HW, C, st)
    G.check()
    return {"out": out, "dx": dx}


def bce_rows_case(L, n, t_offset, masked, rows=2):
    """vp_bce_rows_f32 and vp_bce_masked_rows_bwd_f32; t starts t_offset floats past a 16-byte boundary (p starts on one)"""
    P, st = _env()
    G, o = Guards(), {}
    p = probs(n + t_offset, rows, n)
    t = _u(n + 11, rows * n + 4)[t_offset:t_offset + rows * n]
    mask = (_u(n + 12, rows, n) > 0.3).float() if masked else None
    nb = L.h.vp_bce_rows_workspace_bytes(rows, n)
    o["ws_bytes"] = torch.tensor([nb, L.h.vp_bce_masked_rows_bwd_workspace_bytes(rows, n)])
    ws, _ = G.ws("ws", nb)
    o["rows"] = G.out("rows", rows)
    L.call("vp_bce_rows_f32", P(p), P(t), rows, n, P(o["rows"]), P(ws), nb, st)
    ws, _ = G.ws("ws", nb)
    o["masked rows"], o["dlogit"] = G.out("mrows", rows), G.out("dlogit", rows, n)
    L.call("vp_bce_masked_rows_bwd_f32", P(p), P(t), P(mask), rows, n, P(o["masked rows"]), P(o["dlogit"]), P(ws), nb, st)
    G.check()
    return o


def transpose_case(L, rows, cols, B=2):
    """NCHW [B][rows][cols] -> NHWC and back, with the split planes in both formats"""
    P, st = _env()
    G, o = Guards(), {}
    x = _r(rows * 100 + cols, B, rows, cols)
    n = B * rows * cols
    o["nhwc"] = G.out("nhwc", n)
    L.call("vp_nchw_to_nhwc_f32", P(x), P(o["nhwc"]), B, rows, cols, 1, st)
    o["split y"], o["split planes"] = G.out("y", n), G.planes("ys", n)
    L.call("vp_nchw_to_nhwc_split_f32", P(x), P(o["split y"]), P(o["split planes"]), B, rows, cols, 1, st)
    for fmt in (0, 1):
        o[f"fmt{fmt} planes"] = G.planes("ys", n)
        L.call("vp_nchw_to_nhwc_split_fmt_f32", P(x), None, P(o[f"fmt{fmt} planes"]), B, rows, cols, 1, fmt, st)
    o["nchw"] = G.out("nchw", n)
    L.call("vp_nhwc_to_nchw_f32", P(x), P(o["nchw"]), B, cols, rows, 1, st)
    G.check()
    return o


def upsample_case(L, H, W, C, B=2):
    P, st = _env()
    G = Guards()
    s = H * 100 + W * 10 + C
    x, dy = _r(s, B, H, W, C), _r(s + 1, B, 2 * H, 2 * W, C)
    y, dx = G.out("y", B, 2 * H, 2 * W, C), G.out("dx", B, H, W, C)
    L.call("vp_upsample2x_bilinear_fwd_f32", P(x), P(y), B, H, W, C, st)
    L.call("vp_upsample2x_bilinear_bwd_f32", P(dy), P(dx), B, H, W, C, st)
    G.check()
    return {"y": y, "dx": dx}


def _cases():
    c = [(flat_case, (n,), False) for n in FLAT_N + [FLAT_BIG, QUAD_BIG]]
    c += [(channels_case, (n,), False) for n in FLAT_N + [FLAT_BIG]]
    c += [(reduce_case, (n,), True) for n in FLAT_N + [REDUCE_BIG]]
    c += [(rmsprop_case, (n,), False) for n in FLAT_N + [REDUCE_BIG]]
    c += [(adam_case, (n, step, gs), False) for n in ADAM_N for step, gs in ((3, 1.0), (4, 0.25))]
    c += [(adam_outer_case, s, False) for s in ADAM_OUTER]
    c += [(latent_adam_case, (rows, Z, pw), True) for rows in (1, 3) for Z in (1, 63, 64, 65, 130) for pw in (0.0, 1.0)]
    c += [(be_case, (B, n), True) for B in (1, 3) for n in (1, 4095, 4096, 4097, 8193)]
    c += [(rowsum_case, (n,), True) for n in (1, 255, 256, 257, 511, 512, 513)]
    c += [(gan_head_case, (B,), True) for B in (1, 5, 64, 100)]
    c += [(smooth_l1_case, s, True) for s in ((1, 1, 0), (3, 5, 2), (40, 7, 6))]
    c += [(softmax_case, (R, n), True) for R in (1, 4, 5) for n in (1, 63, 64, 65, 130)]
    c += [(cross_entropy_case, (R, n), True) for R in (1, 255, 256, 257) for n in (1, 10)]
    c += [(cross_entropy_case, (105000, 10), True)]                                     # the backward kernel's second trip
    c += [(latent_case, (B, Z), True) for B in (1, 3) for Z in (1, 63, 64, 65, 130)]
    c += [(latent_case, (2, 300000), True)]                                             # latent_bwd's second trip
    c += [(avgpool_case, (C, HW), True) for C in (1, 63, 64, 65) for HW in (1, 3, 4, 5)]
    c += [(avgpool_case, (128, 4099), True)]                                            # the backward kernel's second trip
    c += [(bce_rows_case, (n, off, masked), True) for n in (1, 4095, 4096, 4097, 8195) for off in (0, 1) for masked in (True, False)]
    c += [(transpose_case, (r, k), False) for r in (1, 31, 32, 33) for k in (1, 31, 32, 33)]
    c += [(upsample_case, (H, W, C), False) for H in (1, 2, 3) for W in (1, 2, 3) for C in (1, 3)]
    c += [(upsample_case, (128, 128, 33), False)]                                       # both kernels' second trips
    return c


CASES = _cases()
