"""Structure of the fused VAE-GAN inference plan (vae_play_amd.infer_gan.FusedVAEGANInference), checked without a GPU: the plan is
built over host buffers (``_plan_only=True``) and never run."""
import pytest

# tests/test_infer_plan.py's tuples: what an inference plan must never launch, and what belongs to refresh()
FORBIDDEN = ("wgrad", "_bwd", "vp_bn_stats", "vp_bn_small_fwd", "_stats_", "loss", "vp_bce", "vp_adam", "vp_rmsprop", "vp_colsum",
             "vp_sum_f32", "slab_reduce")
PREP_ONLY = ("vp_pack_", "vp_bn_fold_f32", "vp_split_f32", "vp_split_pad_f32", "vp_split_fmt_f32")
S, Z, B = 32, 16, 4
GAN_LISTS = {"gan.params", "gan.forward", "gan.discriminate", "gan.similarity"}


def _net():
    import torch
    import vae_play_amd as V
    torch.manual_seed(0)
    return V.VaeGan(S, Z)


def _calls(inf, which):
    return [c for plan in inf._plans[which] for c in plan.calls]


def _names(inf, which):
    return [c[0] for c in _calls(inf, which)]


def _snapshot(inf):
    """every list as (name, argument values): pointers by address"""
    return {w: [(c[0], tuple(getattr(a, "value", a) for a in c[2])) for c in _calls(inf, w)] for w in inf._plans}


def test_a_plan_without_gan_lists_is_the_parents():
    import vae_play_amd as V
    net = _net()
    inf = V.FusedVAEGANInference(net, B, _plan_only=True)
    ref = V.FusedVAEInference.from_modules(net.encoder, net.decoder, B, S, 1, _plan_only=True)
    assert isinstance(inf, V.FusedVAEInference) and (inf.S, inf.C, inf.Z, inf.L) == (S, 1, Z, 2)
    assert set(inf._plans) == set(ref._plans) == {"encode", "decode", "reconstruct"}
    assert list(inf._bufs) == list(ref._bufs)
    assert all(inf._bufs[k].shape == ref._bufs[k].shape and inf._bufs[k].dtype == ref._bufs[k].dtype for k in ref._bufs)
    for w in ref._plans:
        assert _names(inf, w) == _names(ref, w)
        # the same launches with the same scalar arguments (the pointers are other allocations)
        for a, b in zip(_calls(inf, w), _calls(ref, w)):
            assert [x for x in a[2] if not hasattr(x, "value")] == [x for x in b[2] if not hasattr(x, "value")], a[0]
    assert [c[0] for c in inf._prep.calls] == [c[0] for c in ref._prep.calls]


def test_enable_gan_adds_lists_and_leaves_the_parents_alone():
    import vae_play_amd as V
    from vae_play_amd import _lib
    net = _net()
    inf = V.FusedVAEGANInference(net, B, _plan_only=True)
    before, bufs_before, prep_before = _snapshot(inf), dict(inf._bufs), [c[0] for c in inf._prep.calls]
    inf.enable_gan()
    inf.enable_gan()                                             # (idempotent)
    assert set(inf._plans) == {"encode", "decode", "reconstruct"} | GAN_LISTS
    after = _snapshot(inf)
    assert all(after[w] == before[w] for w in before), "enable_gan() changed a list of the parent"
    assert [c[0] for c in inf._prep.calls] == prep_before
    new = set(inf._bufs) - set(bufs_before)
    assert new and all(k.startswith("gan.") for k in new), sorted(new)
    assert all(inf._bufs[k] is bufs_before[k] for k in bufs_before)
    for which in GAN_LISTS:
        for c in _calls(inf, which):
            name, args, side = c[0], c[2], c[6]
            assert name in _lib.SIGNATURES, name
            assert len(args) == len(_lib.SIGNATURES[name][1]), name
            assert side is None, f"{name}: inference plans are single-stream"
            assert not any(f in name for f in FORBIDDEN), f"{which}: {name} is a training launch"
            assert not any(name.startswith(f) for f in PREP_ONLY), f"{which}: {name} belongs to refresh()"
    for c in inf._gan.prep.calls:
        assert c[0] in _lib.SIGNATURES and len(c[2]) == len(_lib.SIGNATURES[c[0]][1]) and c[6] is None, c[0]
    assert inf._n_side_events == 0


def test_structure_of_the_gan_lists():
    import vae_play_amd as V
    net = _net()
    inf = V.FusedVAEGANInference(net, B, _plan_only=True)
    inf.enable_gan()
    assert _names(inf, "gan.forward") == _names(inf, "reconstruct") + _names(inf, "gan.params")
    assert all(a is b for a, b in zip(inf._plans["gan.forward"], inf._plans["reconstruct"])), "the parent's _Plan objects themselves"
    assert _names(inf, "gan.params") == ["vp_gemm_f32"]
    gemm = _calls(inf, "gan.params")[0][2]
    assert gemm[9:13] == [B, 3, Z, 0] and gemm[8] is not None          # M, N = 3, K, mode; the folded bias
    prep = [c[0] for c in inf._gan.prep.calls]
    n_bn = sum(1 for m in net.discriminator.modules() if hasattr(m, "num_batches_tracked"))
    assert n_bn == net.iter_level + 1
    assert prep.count("vp_bn_fold_f32") == n_bn
    assert prep.count("vp_lin_fold_f32") == 6
    assert prep.count("vp_pack_w5_batch") == 1 and prep[0] == "vp_pack_w5_batch"
    assert set(prep) == {"vp_pack_w5_batch", "vp_bn_fold_f32", "vp_lin_fold_f32"}
    # the fold's shapes, from the output side: (M, N, K)
    folds = [tuple(c[2][4:7]) for c in inf._gan.prep.calls if c[0] == "vp_lin_fold_f32"]
    assert folds == [(1, 32, 64), (2, 32, 64), (3, 64, 128), (3, 128, 256), (3, 256, 512), (3, 512, Z)]
    last = [c for c in inf._gan.prep.calls if c[0] == "vp_lin_fold_f32"][-1][2]
    assert last[7].value == inf._bufs["gan.w_eff"].data_ptr() and last[8].value == inf._bufs["gan.b_eff"].data_ptr()


@pytest.mark.parametrize("size,z", [(16, 8), (32, 16), (64, 32)])
def test_discriminator_lists(size, z):
    import torch
    import vae_play_amd as V
    torch.manual_seed(0)
    net = V.VaeGan(size, z)
    L = net.iter_level
    inf = V.FusedVAEGANInference(net, B, _plan_only=True)
    inf.enable_gan()
    for which in ("gan.discriminate", "gan.similarity"):
        calls = _calls(inf, which)
        names = [c[0] for c in calls]
        assert names.count("vp_conv5_smallin_fwd_planes_bf16x3") == 2
        assert "vp_split_f32" not in names and "vp_conv5_smallin_fwd_bf16x3" not in names
        i0 = names.index("vp_conv5_smallin_fwd_planes_bf16x3")
        assert names[i0 + 1] == "vp_conv5_smallin_fwd_planes_bf16x3"
        disc = names[i0 + 2:]
        # L - 1 blocks before the tap (one or two launches each), the tap block's plain convolution, the tap, fc.0, the head
        t = disc.index("vp_disc_tap_eval_f32")
        assert disc[t - 1] == "vp_conv5_gather_bf16x3" and "_affine_" not in disc[t - 1]
        tail = ["vp_disc_tap_eval_f32", "vp_gemm_f32", "vp_disc_head_eval_f32"] + (["vp_half_sqdiff_rowsum_f32"] if which == "gan.similarity" else [])
        assert disc[t:] == tail, disc[t:]
        assert "vp_nhwc_to_nchw_f32" not in disc
        body = calls[i0 + 2:i0 + 2 + t - 1]                    # the blocks before the tap
        assert len({c[5].split(".fwd")[0].split(".bn")[0] for c in body}) == L - 1
        # no normalise pass for the tap block or fc.1
        assert not [c for c in calls[i0:] if c[0].startswith("vp_bn_act_fwd") and (f"disc{L}" in c[5] or ".fc" in c[5])]
        assert len([n for n in disc if n.startswith("vp_bn_act_fwd")]) <= L - 1
        # the two stem launches write the two halves of one split tensor
        a, b = calls[i0][2], calls[i0 + 1][2]
        ys = inf._bufs["gan.disc0.ys"]
        half = B * size * size * 32
        assert ys.shape == (2, 2 * half)
        assert a[3].value == ys.data_ptr() and b[3].value == ys.data_ptr() + 2 * half and a[4] == b[4] == 2 * half
        assert a[5:11] == b[5:11] == [B, size, size, 1, 32, 1]
        tap = calls[i0 + 2 + t][2]
        if which == "gan.discriminate":
            x = inf._bufs["gan.x"]
            assert x.shape == (2 * B, 1, size, size)
            assert a[0].value == x.data_ptr() and b[0].value == x.data_ptr() + 4 * B * size * size
            assert tap[6].value == inf._bufs["gan.features"].data_ptr() and tap[7] == 0 and tap[8] is None
        else:
            assert a[0].value == inf.x_nchw.data_ptr()
            assert b[0].value == inf._xt_nhwc.data_ptr(), "half b reads the decode list's output where it lies"
            fin = [c for c in _calls(inf, "decode") if c[5] == "fin.fwd"][0]
            assert any(getattr(v, "value", None) == inf._xt_nhwc.data_ptr() for v in fin[2])
            assert tap[6] is None and tap[7] == B and tap[8].value == inf._bufs["gan.mse"].data_ptr()
        assert tap[3:5] == [2 * B, 32 << L]
    # similarity = encode, the reparameterisation, decode, params, then the discriminator section
    sim = _names(inf, "gan.similarity")
    head = _names(inf, "encode") + ["vp_latent_fwd_f32"] + _names(inf, "decode") + ["vp_gemm_f32"]
    assert sim[:len(head)] == head and sim[len(head)] == "vp_conv5_smallin_fwd_planes_bf16x3"


@pytest.mark.parametrize("prec", ("f32", "f16"))
def test_other_precisions_build_params_and_refuse_the_discriminator(prec):
    import torch
    import vae_play_amd as V
    net = _net()
    inf = V.FusedVAEGANInference(net, B, precision=prec, _plan_only=True)
    inf.enable_gan()
    assert {w for w in inf._plans if w.startswith("gan.")} == {"gan.params", "gan.forward"}
    assert _names(inf, "gan.params") == ["vp_gemm_f32"]
    assert _names(inf, "gan.forward") == _names(inf, "reconstruct") + ["vp_gemm_f32"]
    prep = [c[0] for c in inf._gan.prep.calls]
    assert prep == ["vp_lin_fold_f32"] * 6
    x = torch.zeros(1, 1, S, S)
    for call in (lambda: inf.discriminate(x), lambda: inf.similarity(x)):
        with pytest.raises(NotImplementedError, match="bf16x3"):
            call()
