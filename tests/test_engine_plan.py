"""Structure of the fused steps' launch plans, checked without a GPU (the plans are built over host buffers and never run): every
launch resolves to a symbol of the C ABI with as many arguments as it declares, every parameter's gradient slice -- and, for the
VAE-GAN decoder, its slice of the shadow arena of the second pass -- is an argument of some backward launch, every wait for a side
event follows the launch that records it, and every named point the steps' callbacks use occurs exactly once."""
import pytest

VAE_CASES = [(prec, C, S, z, B) for prec in ("f32", "bf16x3", "f16x2") for (C, S, z, B) in ((1, 32, 16, 4), (3, 128, 128, 4))]


def _launch_pointers(plan):
    return {a.value for c in plan.calls for a in c[2] if hasattr(a, "value") and a.value}


def _check_plans(plans, hook_names):
    from vae_play_amd import _lib
    recorded = set()
    hooks = []
    for plan in plans:                        # in run order
        for c in plan.calls:
            name, args, side = c[0], c[2], c[6]
            if name == "__hook__":
                hooks.append(args[0])
            elif name == "__wait_side__":
                # (a wait for an event that was never recorded would be skipped at run time)
                assert args[0] in recorded, f"wait_side({args[0]}) before any launch records it"
            else:
                assert name in _lib.SIGNATURES, name
                assert len(args) == len(_lib.SIGNATURES[name][1]), name
                if side is not None:
                    recorded.add(side)
    for key in hook_names:
        assert hooks.count(key) == 1, key
    return recorded


@pytest.mark.parametrize("prec,C,S,z,B", VAE_CASES)
def test_vae_plan_structure(prec, C, S, z, B):
    import torch
    import vae_play_amd as V
    from vae_play_amd import optim
    from vae_play_amd.engine import FusedVAEStep
    torch.manual_seed(0)
    vae = V.VAE(S, z, C).train()
    opt = optim.Adam(vae.parameters(), lr=1e-4)
    st = FusedVAEStep(vae, opt, B, S, C, precision=prec, _plan_only=True)
    hooks = ["fwd_done", "dec_done", "fc_wgrad", "enc_dense_done"] + (["enc_tail"] if prec != "f32" else [])
    recorded = _check_plans([st._fwd, st._bwd], hooks)
    assert recorded == set(range(st._n_side_events))
    assert (st._n_side_events > 0) == (prec != "f32") and (st._enc_tail_first is not None) == (prec != "f32")
    if st._bwd_b_enc_tail is not None:
        assert st._bwd.calls[st._bwd_b_enc_tail][0] == "__hook__" and st._bwd.calls[st._bwd_b_enc_tail][2][0] == "enc_tail"
    ptrs = _launch_pointers(st._bwd)
    for n, p in vae.named_parameters():
        assert opt.arena.grad_view(p).data_ptr() in ptrs, n
    # the "fc_wgrad" hook stands in for exactly the GEMM that writes encoder.fc.0's weight gradient
    i = next(j for j, c in enumerate(st._bwd.calls) if c[0] == "__hook__" and c[2][0] == "fc_wgrad")
    assert st._bwd.calls[i][2][1]
    nxt = st._bwd.calls[i + 1]
    assert nxt[0] == "vp_gemm_f32" and nxt[2][6].value == opt.arena.grad_view(vae.encoder.fc[0].weight).data_ptr()
    # the buffers the GPU accuracy tests read
    L = vae.iter_level
    for name in ["enc.hb", "dec.db"] + [f"dec{L - 1}.u", f"enc{L - 1}.a"]:
        assert name in st._bufs, name


@pytest.mark.parametrize("S,z,B", [(32, 16, 4), (128, 128, 16)])
def test_gan_plan_structure(S, z, B):
    import vae_play_amd as V
    from vae_play_amd import optim
    from vae_play_amd.engine_gan import FusedVAEGANStep
    net = V.VaeGan(S, z).train()
    opts = [optim.RMSprop(m.parameters(), lr=1e-4) for m in (net.encoder, net.decoder, net.discriminator, net.param_encoder)]
    st = FusedVAEGANStep(net, opts, B, S, _plan_only=True)
    recorded = _check_plans([st._fwd, st._fwd_disc, st._bwd], ["disc_done", "dec_done", "enc_dense_done"])
    assert recorded == set(range(st._n_side_events)) and st._n_side_events > 0
    ptrs = _launch_pointers(st._bwd)
    dec_ids = {id(p) for p in net.decoder.parameters()}
    for n, p in net.named_parameters():
        assert p._vp_arena.grad_view(p).data_ptr() in ptrs, n
        if id(p) in dec_ids:
            assert st._dec_shadow.data_ptr() + 4 * p._vp_off in ptrs, n + " (second decoder pass)"
    # BatchNorm forward passes per step: decoder layers run twice (z, z_p), discriminator blocks count both reference calls
    counts = {}
    for bn, c in st._bn_counts:
        counts[id(bn)] = counts.get(id(bn), 0) + c
    for m in net.decoder.modules():
        if hasattr(m, "num_batches_tracked"):
            assert counts[id(m)] == 2
    for m in net.encoder.modules():
        if hasattr(m, "num_batches_tracked"):
            assert counts[id(m)] == 1
    assert counts[id(net.discriminator.fc[1])] == 1
    for blk in list(net.discriminator.conv)[1:]:
        assert counts[id(blk.bn)] == 2
    # the two loss coefficients as fp32 accumulation forms them
    assert abs(st.c_disc - 1e-6) < 2e-8 and st.c_disc != 1e-6
    assert abs(st.c_mse - 1.000001) < 1e-7
