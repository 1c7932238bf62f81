"""Glue between the VAE-GAN inference tests and the fp64 oracle (oracle/ref_vaegan.py, imported as it is): a VaeGan with non-trivial
eval state, seeded batches, and the eval-mode pipeline of ``similarity`` written with the oracle's functions."""
import torch

DEV = "cuda"


def trained_vaegan(S, z, B, seed=0):
    """a VaeGan whose eval state cannot hide a dropped or swapped constant: every BatchNorm's gamma ~ U(0.5, 1.5) and beta ~ N(0, 0.2),
    every other bias ~ N(0, 0.1) (the reference initialises them to zero: param_encoder, discriminator.conv.0.0, discriminator.fc.3),
    then three train-mode forwards on seeded batches in "f32" (momentum 0.9 moves the running statistics to the data's); eval mode"""
    import vae_play_amd as V
    torch.manual_seed(seed)
    net = V.VaeGan(S, z).to(DEV)
    g = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        bn_params = set()
        for m in net.modules():
            if hasattr(m, "num_batches_tracked"):
                m.weight.copy_(torch.empty(m.weight.shape).uniform_(0.5, 1.5, generator=g))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                bn_params.add(id(m.bias))
        for name, p in net.named_parameters():
            if name.endswith(".bias") and id(p) not in bn_params:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        net.train()
        V.set_conv_precision("f32")
        for k in range(3):
            xb = torch.rand((B, 1, S, S), generator=torch.Generator().manual_seed(200 + k)).to(DEV)
            eb = torch.randn((B, z), generator=torch.Generator().manual_seed(300 + k)).to(DEV)
            zp = torch.randn((B, z), generator=torch.Generator().manual_seed(400 + k)).to(DEV)
            net(xb, eps=eb, z_p=zp)
    torch.cuda.synchronize()
    return net.eval()


def batch(S, z, n, seed=7):
    x = torch.rand((n, 1, S, S), generator=torch.Generator().manual_seed(seed))
    eps = torch.randn((n, z), generator=torch.Generator().manual_seed(seed + 1))
    return x, eps


def state(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}, {n: m.training for n, m in net.named_modules()}


def loss_terms(x, x_tilde, feat, p):
    """the per-image terms of ``similarity`` from (x, x_tilde), the features (2n, F) and the scores (2n,) of (x | x_tilde), in the
    dtype given (VaeGan.loss, models/networks.py:265-276)"""
    n = len(x)
    return {"nle": (0.5 * (x.reshape(n, -1) - x_tilde.reshape(n, -1)) ** 2).sum(1),
            "mse": (0.5 * (feat[:n] - feat[n:]) ** 2).sum(1),
            "bce_dis_original": -torch.log(p[:n] + 1e-3), "bce_dis_predicted": -torch.log(1 - p[n:] + 1e-3)}


def oracle_similarity(net, x, eps):
    """everything ``forward`` / ``discriminate`` / ``similarity`` return, from the fp64 oracle in eval mode on the model's state"""
    from oracle import ref_cpu as O
    from oracle import ref_vaegan as RV
    L = net.iter_level
    p64 = {k: (v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu().clone()) for k, v in net.state_dict().items()}
    x, eps = x.double(), eps.double()
    with torch.no_grad():
        mu, logvar = O.encoder_forward(p64, x, L, False)
        z = O.reparameterize(mu, logvar, eps)
        xt = O.decoder_forward(p64, z, L, False)
        out = {"mu": mu, "logvar": logvar, "x_tilde": xt, "params": RV.direct_decoder_forward(p64, z)}
        none = x[:0]
        out["features"] = RV.discriminator_forward(p64, x, xt, none, "REC", L, L, training=False)
        out["p"] = RV.discriminator_forward(p64, x, xt, none, "GAN", L, L, training=False).reshape(-1)
        out["logit"] = torch.logit(out["p"])
        out.update(loss_terms(x, xt, out["features"], out["p"]))
    return out


def modules_similarity(net, x, eps):
    """the same from the drop-in modules in eval mode under set_conv_precision("bf16x3"), the loss terms with torch"""
    import vae_play_amd as V
    V.set_conv_precision("bf16x3")
    try:
        with torch.no_grad():
            xt, params = net(x, eps=eps)
            feat, p = net.discriminator.forward_rec_and_gan(x, xt, x[:0])
    finally:
        V.set_conv_precision("f32")
    p = p.reshape(-1)
    out = {"x_tilde": xt, "params": params, "features": feat, "p": p, "logit": torch.logit(p.double())}
    out.update(loss_terms(x, xt, feat, p))
    return out
