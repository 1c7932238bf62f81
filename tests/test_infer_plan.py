"""Structure of the fused inference plans (vae_play_amd.infer.FusedVAEInference), checked without a GPU: the plans are built over
host buffers (``_plan_only=True``) and never run; the library's support / workspace queries are host code."""
import pytest

CASES = [(prec, C, S, z, B) for prec in ("bf16x3", "f32") for (C, S, z, B) in ((1, 32, 16, 4), (3, 64, 64, 4), (3, 128, 128, 32))]

# what an inference plan must never launch: weight gradients, BatchNorm backward / batch statistics, losses, optimisers
FORBIDDEN = ("wgrad", "_bwd", "vp_bn_stats", "vp_bn_small_fwd", "_stats_", "loss", "vp_bce", "vp_adam", "vp_rmsprop", "vp_colsum",
             "vp_sum_f32", "slab_reduce")
# weight packing / folding belongs to refresh(), not to a call
PREP_ONLY = ("vp_pack_", "vp_bn_fold_f32", "vp_split_f32", "vp_split_pad_f32", "vp_split_fmt_f32")


def _build(prec, C, S, z, B):
    import torch
    import vae_play_amd as V
    torch.manual_seed(0)
    vae = V.VAE(S, z, C)
    return vae, V.FusedVAEInference(vae, B, S, C, precision=prec, _plan_only=True)


def _calls(inf, which):
    return [c for plan in inf._plans[which] for c in plan.calls]


@pytest.mark.parametrize("prec,C,S,z,B", CASES)
def test_inference_plan_structure(prec, C, S, z, B):
    from vae_play_amd import _lib
    vae, inf = _build(prec, C, S, z, B)
    assert set(inf._plans) == {"encode", "decode", "reconstruct"}
    for which in inf._plans:
        for c in _calls(inf, which):
            name, args, side = c[0], c[2], c[6]
            assert name in _lib.SIGNATURES, name                          # (no hooks, no side-stream waits either)
            assert len(args) == len(_lib.SIGNATURES[name][1]), name
            assert side is None, f"{name}: inference plans are single-stream"
            assert not any(f in name for f in FORBIDDEN), f"{which}: {name} is a training launch"
            assert not any(name.startswith(f) for f in PREP_ONLY), f"{which}: {name} belongs to refresh()"
    assert inf._n_side_events == 0
    # reconstruct = encode + the reparameterisation + decode
    names = lambda w: [c[0] for c in _calls(inf, w)]      # noqa: E731
    assert names("reconstruct") == names("encode") + ["vp_latent_fwd_f32"] + names("decode")
    # refresh(): one batched weight pack, the first block's im2col weight, one fold per BatchNorm -- and nothing that touches activations
    prep = [c[0] for c in inf._prep.calls]
    assert prep.count("vp_pack_w5_batch") == 1
    n_bn = sum(1 for m in vae.modules() if hasattr(m, "num_batches_tracked"))
    assert prep.count("vp_bn_fold_f32") == n_bn
    assert all(any(n.startswith(f) for f in PREP_ONLY) for n in prep), prep
    for c in inf._prep.calls:
        assert len(c[2]) == len(_lib.SIGNATURES[c[0]][1]), c[0]
    # no launch writes into the module: no argument of a per-call launch is a BatchNorm running buffer's variance ... the running
    # mean is read by the separate normalise passes; parameters are read-only operands.  (The GPU tests compare the bits.)
    rv = {m.running_var.data_ptr() for m in vae.modules() if hasattr(m, "num_batches_tracked")}
    for which in inf._plans:
        for c in _calls(inf, which):
            assert not rv & {a.value for a in c[2] if hasattr(a, "value") and a.value}, c[0]


@pytest.mark.parametrize("prec", ("bf16x3", "f32"))
def test_every_statistics_fusing_layer_is_one_launch(prec):
    """At 128x128x3 batch 32: every BatchNorm-followed 5x5 layer whose TRAINING launch fuses the statistics is exactly one launch
    here, without a normalise pass; the separate normalise passes left are exactly the layers the library reports as unfusable
    (plus the first block, which is a 1x1 layer over its im2col, not a 5x5 implicit GEMM)."""
    from vae_play_amd import _lib
    lib = _lib.load()
    C, S, z, B = 3, 128, 128, 32
    vae, inf = _build(prec, C, S, z, B)
    L = vae.iter_level
    stats_ws = lib.vp_conv5_stats_workspace_bytes if prec == "bf16x3" else lib.vp_conv5_stats_f32_workspace_bytes
    enc_ch = [C] + [blk.conv.weight.shape[0] for blk in vae.encoder.conv]
    dec_ch = [vae.decoder._c0] + [blk.conv.weight.shape[1] for blk in list(vae.decoder.conv)[:L]]
    layers = {}      # tag -> (family, B, Hs, Ws, Cbig, Csmall, stride)
    for i in range(1, L):
        layers[f"enc{i}"] = (0, B, S >> (i + 1), S >> (i + 1), enc_ch[i], enc_ch[i + 1], 2)
    for i in range(L):
        layers[f"dec{i}"] = (1, B, 8 << i, 8 << i, dec_ch[i + 1], dec_ch[i], 2)
    calls = _calls(inf, "reconstruct")
    by_tag = {}
    for c in calls:
        if c[5]:
            by_tag.setdefault(c[5].split(".")[0], []).append(c[0])
    n_stats = n_unfusable = 0
    for tag, q in layers.items():
        fuses_stats = stats_ws(*q) != 0
        supported = bool(lib.vp_conv5_affine_supported(q[0], 0 if prec == "bf16x3" else 1, *q[1:]))
        launches = by_tag[tag]
        if fuses_stats:
            n_stats += 1
            assert supported, f"{tag}: the training plan fuses its statistics, the inference launch must fuse its BatchNorm"
        if supported:
            assert len(launches) == 1 and "_affine_" in launches[0], (tag, launches)
            assert not any("vp_bn_act_fwd" in n for n in launches)
        else:
            n_unfusable += 1
            assert len(launches) == 2 and "vp_bn_act_fwd" in launches[1] and "_affine_" not in launches[0], (tag, launches)
    assert n_stats >= (6 if prec == "bf16x3" else 4)         # "the six layers that do not split K" of the training plan
    # the separate normalise passes of 4-D activations that remain: the unfusable 5x5 layers + the first block
    passes_4d = [c for c in calls if c[0].startswith("vp_bn_act_fwd") and c[5].startswith(("enc", "dec")) and ".fc" not in c[5]]
    assert len(passes_4d) == n_unfusable + 1
    assert sorted(inf.unfused_layers) == sorted([t for t, q in layers.items()
                                                 if not lib.vp_conv5_affine_supported(q[0], 0 if prec == "bf16x3" else 1, *q[1:])] + ["enc0"])
    # the last decoder block feeds the final convolution in fp32: its fused launch writes no planes
    last = next(c for c in calls if c[5] == f"dec{L - 1}.fwd")
    assert last[2][4] is not None and last[2][5] is None
    if prec == "bf16x3":      # ... and the fused launches in between write planes only
        mid = next(c for c in calls if c[5] == "dec1.fwd")
        assert mid[2][4] is None and mid[2][5] is not None


def test_vaegan_halves_and_argument_errors():
    import torch
    import vae_play_amd as V
    torch.manual_seed(0)
    net = V.VaeGan(32, 16)
    inf = V.FusedVAEInference.from_modules(net.encoder, net.decoder, 4, 32, 1, _plan_only=True)
    assert inf.C == 1 and inf.Z == 16 and inf.L == 2 and len(_calls(inf, "decode")) > 0
    vae = V.VAE(32, 16, 1)
    with pytest.raises(ValueError, match="precision"):
        V.FusedVAEInference(vae, 4, 32, 1, precision="f16x2", _plan_only=True)
    with pytest.raises(ValueError, match="channel"):
        V.FusedVAEInference(vae, 4, 32, 3, _plan_only=True)
    with pytest.raises(ValueError, match="do not fit"):
        V.FusedVAEInference(vae, 4, 64, 1, _plan_only=True)
    # a plan never runs on host tensors: without _plan_only a CPU model is refused
    from vae_play_amd import _lib
    with pytest.raises(_lib.VaePlayHipError):
        V.FusedVAEInference(vae, 4, 32, 1)
    with pytest.raises(_lib.VaePlayHipError, match="HIP device"):
        inf.decode(torch.zeros(2, 16))


def test_affine_support_query_is_host_code():
    from vae_play_amd import ops
    assert ops.conv5_affine_supported(0, "bf16x3", 32, 32, 32, 64, 128, 2)
    assert ops.conv5_affine_supported(1, "f32", 32, 64, 64, 64, 128, 2)
    assert not ops.conv5_affine_supported(0, "bf16x3", 32, 8, 8, 256, 512, 2)       # the plain launch splits K
    assert not ops.conv5_affine_supported(0, "bf16x3", 32, 32, 32, 64, 128, 3)      # stride
    assert not ops.conv5_affine_supported(2, "bf16x3", 32, 32, 32, 64, 128, 2)      # family
