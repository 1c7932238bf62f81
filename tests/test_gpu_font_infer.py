"""Fused font U-Net inference on the GPU (csrc/font_infer.hip, vae_play_amd.infer_font.FusedFontInference): the new kernels through the C
ABI against fp64, the whole plan against the fp64 oracle next to the module path in ``.eval()``, and the properties that need no
oracle.  Cases, seeded nets and oracle results: tests/font_infer_ref.py."""
import pytest
import torch
import torch.nn.functional as F

from tests import font_infer_ref as R
from tests.guarded import Guards, api, same_bits, tensor_close
from tests.test_gpu_infer import FLOOR
from tests.util import NORTH_STAR_RTOL, record, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
VP_ERR_ARG = -1
ACTS = {None: 0, "relu": 1, "lrelu": 2}
SENTINEL = 7777.0


def _p(t, offset_floats=0):
    from ctypes import c_void_p
    return None if t is None else c_void_p(t.data_ptr() + 4 * offset_floats)


def _conv_in(lib, _lib, x, wp, y, ldy, geom, act, first_channel=0):
    B, H, W, Cin, Cout, ks, stride = geom
    _lib.check(lib.vp_conv_in_act_f32(_p(x), _p(wp), _p(y, first_channel), ldy, B, H, W, Cin, Cout, ks, stride, 1e-5, ACTS[act], R.LRELU, None),
               "vp_conv_in_act_f32")


def _packed(lib, _lib, g, w):
    Cout, Cin, ks, _ = w.shape
    wp = g.out("w_packed", Cout, ks * ks, Cin)
    wd = w.to(DEV)
    _lib.check(lib.vp_conv_in_pack_f32(_p(wd), _p(wp), Cout, Cin, ks, None), "pack")
    torch.cuda.synchronize()
    assert torch.equal(wp.cpu(), w.permute(0, 2, 3, 1).reshape(Cout, ks * ks, Cin))
    return wp


# ---- 1. the whole-image convolution + InstanceNorm kernel through the C ABI ------------------------------------------------------
@pytest.mark.parametrize("case", range(len(R.CONV_IN_CASES)))
def test_conv_in_kernel_vs_fp64(case):
    """Dense (ldy = Cout) and into the upper channel slice of a buffer twice as wide (ldy = 2 Cout): fp64 direct sum + InstanceNorm,
    guards, the other slice untouched, exact zeros for the all-zero output channel and the all-zero image."""
    _lib, _, lib = api()
    B, H, W, Cin, Cout, ks, stride, act = R.CONV_IN_CASES[case]
    x, w, ref = R.conv_in_case(case)
    assert lib.vp_conv_in_supported(H, W, Cin, Cout, ks, stride) == 1
    Ho, Wo = ref.shape[2], ref.shape[3]
    g = Guards()
    wp = _packed(lib, _lib, g, w)
    xd = x.to(DEV)
    y = g.out("y dense", B, Ho, Wo, Cout)
    wide = g.state("y wide", torch.full((B, Ho, Wo, 2 * Cout), SENTINEL))
    geom = (B, H, W, Cin, Cout, ks, stride)
    _conv_in(lib, _lib, xd, wp, y, Cout, geom, act)
    _conv_in(lib, _lib, xd, wp, wide, 2 * Cout, geom, act, first_channel=Cout)
    g.check()
    tensor_close(y.permute(0, 3, 1, 2), ref, f"conv_in case {case} {R.CONV_IN_CASES[case]}")
    assert same_bits(wide[..., Cout:], y), "the sliced output differs from the dense one"
    assert bool((wide[..., :Cout] == SENTINEL).all()), "the other channel slice was written"
    assert not torch.isnan(y).any()
    assert bool((y[..., Cout // 3] == 0).all()), "an all-zero output channel must give exact zeros"
    assert bool((y[B // 2] == 0).all()), "an all-zero image must give exact zeros"


def test_conv_in_result_does_not_depend_on_the_slot_or_tile():
    """the same image alone (B = 1), as image 2 of 3 and as image 16 of 17 (the second tile's first slot at 4x4): the same bits"""
    _lib, _, lib = api()
    B, H, W, Cin, Cout, ks, stride, act = R.CONV_IN_CASES[1]
    assert (B, H * W) == (17, 16)
    x, w, _ = R.conv_in_case(1)
    g = Guards()
    wp = _packed(lib, _lib, g, w)
    xd = x.to(DEV)
    img = xd[16:17].contiguous()
    x3 = torch.cat([xd[0:1], img, xd[5:6]]).contiguous()
    y17, y3, y1 = g.out("y17", 17, 16, Cout), g.out("y3", 3, 16, Cout), g.out("y1", 1, 16, Cout)
    for xx, yy, b in ((xd, y17, 17), (x3, y3, 3), (img, y1, 1)):
        _conv_in(lib, _lib, xx, wp, yy, Cout, (b, H, W, Cin, Cout, ks, stride), act)
    g.check()
    assert same_bits(y1[0], y17[16]) and same_bits(y1[0], y3[1]), "a result depends on the slot or tile its image sits in"
    assert same_bits(y3[0], y17[0]) and same_bits(y3[2], y17[5])


def test_conv_in_entry_refuses_what_the_predicate_refuses():
    _lib, _, lib = api()
    x = torch.zeros((2, 8, 8, 64), device=DEV)
    wp = torch.zeros((64, 9, 64), device=DEV)
    y = torch.full((2, 64, 64), float("nan"), device=DEV)
    call = lambda *a: lib.vp_conv_in_act_f32(*a, None)         # noqa: E731
    good = [_p(x), _p(wp), _p(y), 64, 2, 8, 8, 64, 64, 3, 1, 1e-5, 1, 0.0]

    def bad(i, v):
        a = list(good)
        a[i] = v
        return a
    # null and misaligned pointers, ldy < Cout, B = 0, a 48- and a 96-pixel map, Cin 3 and 96, Cout 32, ks 5, stride 3, tanh, sigmoid
    cases = [bad(0, None), bad(1, None), bad(2, None), bad(3, 32), bad(4, 0), bad(5, 6), bad(6, 12), bad(7, 3), bad(7, 96), bad(8, 32),
             bad(9, 5), bad(10, 3), bad(12, 3), bad(12, 4), bad(0, _p(x, 1))]
    for a in cases:
        assert call(*a) == VP_ERR_ARG, a
    assert lib.vp_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(y).all(), "a refused call wrote"


# ---- 2. the heads' output stage and the two strided passes -----------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(8, 8), (5, 7)])
def test_pred_stage_and_strided_passes_vs_fp64(H, W):
    _lib, _, lib = api()
    B, C = 2, 64
    g0 = R.gen(900 + H)
    x = torch.randn((2, B, H, W, C), generator=g0)
    w = (torch.rand((2, 1, C, 3, 3), generator=g0) * 2 - 1) * (3.0 / (9 * C)) ** 0.5
    bias = torch.randn((2, 1), generator=g0) * 0.3
    with torch.no_grad():
        ref = torch.stack([F.conv2d(x[k].permute(0, 3, 1, 2).double(), w[k].double(), bias[k].double(), padding=1) for k in range(2)])
    thr = ref.median().item()
    g = Guards()
    n_par = lib.vp_font_pred_params_floats(C)
    par = g.out("params", 2, n_par)
    keep = [w.to(DEV), bias.to(DEV)]
    for k in range(2):
        _lib.check(lib.vp_font_pred_pack_f32(_p(keep[0][k]), _p(keep[1][k]), _p(par[k]), C, None), "pack")
    xd = x.to(DEV)
    lg, lgb = g.out("logits", 2, B, 1, H, W), g.out("logits head 1 alone", 1, B, 1, H, W)
    mask = torch.full((lg.numel() + 128,), 0xA5, dtype=torch.uint8, device=DEV)
    mt = mask[64:64 + lg.numel()]
    mt.fill_(7)
    _lib.check(lib.vp_font_pred_infer_f32(_p(xd), xd[0].numel(), _p(par), _p(lg), _p(mt), thr, 2, B, H, W, C, None), "pred")
    _lib.check(lib.vp_font_pred_infer_f32(_p(xd[1]), 0, _p(par[1]), _p(lgb), None, 0.0, 1, B, H, W, C, None), "pred x1")
    g.check()
    assert bool((mask[:64] == 0xA5).all()) and bool((mask[64 + lg.numel():] == 0xA5).all()) and int(mt.max()) <= 1
    for k in range(2):
        tensor_close(lg[k], ref[k], f"font pred {H}x{W} head{k}")
    assert same_bits(lgb[0], lg[1]), "a head depends on the launch it is in"
    m = mt.view(lg.shape).bool().cpu()
    assert torch.equal(m, lg.cpu() >= thr)
    clear = (ref - thr).abs() > 2e-5 * ref.abs().max()
    assert (~clear).float().mean().item() <= 0.01
    assert torch.equal(m[clear], (ref >= thr)[clear])

    # the 2x resize into a channel slice: fp64 reference, the bits of the dense entry, the other slice untouched
    u = x[0]
    ud = u.to(DEV)
    ref_up = F.interpolate(u.permute(0, 3, 1, 2).double(), scale_factor=2, mode="bilinear")
    g = Guards()
    dense = g.out("resize dense", B, 2 * H, 2 * W, C)
    wide = g.state("resize wide", torch.full((B, 2 * H, 2 * W, C + 32), SENTINEL))
    _lib.check(lib.vp_upsample2x_bilinear_fwd_f32(_p(ud), _p(dense), B, H, W, C, None), "resize")
    _lib.check(lib.vp_upsample2x_bilinear_fwd_ld_f32(_p(ud), _p(wide), C + 32, B, H, W, C, None), "resize ld")
    # InstanceNorm + ReLU into the upper slice
    ref_in = torch.relu(F.instance_norm(u.permute(0, 3, 1, 2).double(), eps=1e-5))
    nws = lib.vp_instnorm_workspace_bytes(B, H * W, C)
    ws, _ = g.ws("ws", (nws + 3) // 4 * 4)
    mean, rstd = g.out("mean", B, C), g.out("rstd", B, C)
    yd = g.out("in dense", B, H, W, C)
    yw = g.state("in wide", torch.full((B, H, W, 32 + C), SENTINEL))
    _lib.check(lib.vp_instnorm_act_fwd_f32(_p(ud), _p(yd), _p(mean), _p(rstd), B, H * W, C, 1e-5, 1, 0.0, _p(ws), nws, None), "in")
    _lib.check(lib.vp_instnorm_act_fwd_ld_f32(_p(ud), _p(yw, 32), 32 + C, _p(mean), _p(rstd), B, H * W, C, 1e-5, 1, 0.0, _p(ws), nws, None),
               "in ld")
    g.check()
    tensor_close(wide[..., :C].permute(0, 3, 1, 2), ref_up, f"resize ld {H}x{W}")
    assert same_bits(wide[..., :C], dense) and bool((wide[..., C:] == SENTINEL).all())
    tensor_close(yw[..., 32:].permute(0, 3, 1, 2), ref_in, f"instnorm ld {H}x{W}")
    assert same_bits(yw[..., 32:], yd) and bool((yw[..., :32] == SENTINEL).all())


def test_bad_arguments_are_refused_and_launch_nothing():
    _, _, lib = api()
    B, H, W, C = 1, 4, 4, 64
    x = torch.zeros((2, B, H, W, C), device=DEV)
    par = torch.zeros((2, 9 * C + 4), device=DEV)
    lg = torch.full((2, B, H, W), float("nan"), device=DEV)
    y = torch.full((B, 2 * H, 2 * W, 2 * C), float("nan"), device=DEV)
    ws = torch.zeros(4096, device=DEV)
    pr = lambda *a: lib.vp_font_pred_infer_f32(*a, None)       # noqa: E731
    for a in [(None, 0, _p(par), _p(lg), None, 0.0, 2, B, H, W, C), (_p(x), 0, None, _p(lg), None, 0.0, 2, B, H, W, C),
              (_p(x), 0, _p(par), None, None, 0.0, 2, B, H, W, C), (_p(x), 0, _p(par), _p(lg), None, 0.0, 2, B, H, W, 6),
              (_p(x), 0, _p(par), _p(lg), None, 0.0, 2, B, H, W, 260), (_p(x), 0, _p(par), _p(lg), None, 0.0, 0, B, H, W, C),
              (_p(x), 0, _p(par), _p(lg), None, 0.0, 2, 0, H, W, C), (_p(x), 0, _p(par), _p(lg), None, 0.0, 2, B, -1, W, C),
              (_p(x), 2, _p(par), _p(lg), None, 0.0, 2, B, H, W, C)]:
        assert pr(*a) == VP_ERR_ARG, a
    assert lib.vp_last_error()
    assert lib.vp_font_pred_pack_f32(_p(x), _p(x), _p(par), 6, None) == VP_ERR_ARG
    assert lib.vp_font_pred_pack_f32(_p(x), None, _p(par), C, None) == VP_ERR_ARG
    assert lib.vp_upsample2x_bilinear_fwd_ld_f32(_p(x), _p(y), C - 4, B, H, W, C, None) == VP_ERR_ARG
    assert lib.vp_upsample2x_bilinear_fwd_ld_f32(_p(x), None, 2 * C, B, H, W, C, None) == VP_ERR_ARG
    args = (_p(ws), _p(ws), B, H * W, C, 1e-5, 1, 0.0, _p(ws), 4096 * 4, None)
    assert lib.vp_instnorm_act_fwd_ld_f32(_p(x), _p(y), C - 4, *args) == VP_ERR_ARG
    assert lib.vp_instnorm_act_fwd_ld_f32(_p(x), _p(y), 2 * C + 2, *args) == VP_ERR_ARG
    assert lib.vp_instnorm_act_fwd_ld_f32(_p(x), _p(y, 1), 2 * C, *args) == VP_ERR_ARG
    assert lib.vp_font_relay_input_f32(_p(x), _p(x), None, _p(y), B, 16, C, 256, None) == VP_ERR_ARG
    assert lib.vp_font_attn1_f32(_p(x), _p(x), _p(x), _p(y), 0, None) == VP_ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(lg).all() and torch.isnan(y).all() and not par.any(), "a refused call wrote"


# ---- 3. the whole plan -------------------------------------------------------------------------------------------------------------
_DEV_NETS = {}


def _net(S):
    if S not in _DEV_NETS:
        import copy
        net, imgs, y, ref = R.net_case(S)
        _DEV_NETS[S] = (copy.deepcopy(net).to(DEV).eval(), imgs.to(DEV), {k: v.to(DEV) for k, v in y.items()}, ref)
    return _DEV_NETS[S]


@pytest.mark.parametrize("with_y", (False, True), ids=("image", "embed"))
@pytest.mark.parametrize("S", (16, 32))
@pytest.mark.parametrize("prec", ("f32", "bf16x3"))
def test_whole_plan_vs_fp64_oracle(prec, S, with_y):
    """tests/test_gpu_infer.py's rule: every output within NORTH_STAR_RTOL of the fp64 oracle, and err_fused <= max(2 err_modules,
    FLOOR[precision]) with err_modules = the same net in .eval() on the GPU with the same weights; the conditioning vectors too (the
    logits move by ~1e-3 between the two branches: they alone could not show that y was used)."""
    import vae_play_amd as V
    net, x, y, ref = _net(S)
    yy = y if with_y else None
    inf = V.FusedFontInference(net, R.BATCH, precision=prec)
    out = inf.predict(x, yy)
    out["label"], out["style"] = inf.condition(x, yy)
    V.set_conv_precision(prec)
    try:
        with torch.no_grad():
            mod = net(x, yy)
            mod["label"], mod["style"] = net.embeding_block(y["cls"], y["cnt_style"]) if with_y else net.style_encoder(x, x)
    finally:
        V.set_conv_precision("f32")
    torch.cuda.synchronize()
    want = dict(ref["y" if with_y else "none"])
    want["label"], want["style"] = ref["cond_y" if with_y else "cond_none"]
    tag = f"{prec} S{S} {'embed' if with_y else 'image'}"
    fails = []
    for name in ("edges", "masks", "label", "style"):
        assert out[name].shape == want[name].shape
        ef, em = rel_err(out[name], want[name]), rel_err(mod[name], want[name])
        record(f"font infer fused {tag} {name}", ef)
        record(f"font infer modules {tag} {name}", em)
        print(f"{tag} {name}: fused {ef:.3e}  modules {em:.3e}")
        if not ef <= NORTH_STAR_RTOL:
            fails.append(f"{name}: fused {ef:.3e} > {NORTH_STAR_RTOL:.0e}")
        if not ef <= max(2 * em, FLOOR[prec]):
            fails.append(f"{name}: fused {ef:.3e} > max(2 x modules {em:.3e}, floor {FLOOR[prec]:.1e})")
    assert not fails, "; ".join(fails)
    assert net.training is False


# ---- 4. properties that need no oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ("f32", "bf16x3"))
def test_properties_without_oracle(prec):
    import vae_play_amd as V
    S = 16
    net, _, _, ref = _net(S)
    x5 = torch.rand((5, 3, S, S), generator=R.gen(77)).to(DEV)
    y5 = {"cls": F.one_hot(torch.tensor([3, 140, 7, 7, 99]), 143).float().to(DEV), "cnt_style": torch.rand((5, 5), generator=R.gen(78)).to(DEV)}
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    flags = {n: m.training for n, m in net.named_modules()}
    inf = V.FusedFontInference(net, 3, precision=prec)

    # n = 5 through a batch_size 3 plan == the five images one at a time, with and without y
    full, full_y = inf.predict(x5), inf.predict(x5, y5)
    assert full["edges"].shape == full["masks"].shape == (5, 1, S, S)
    for k in ("edges", "masks"):
        assert same_bits(full[k], torch.cat([inf.predict(x5[i:i + 1])[k] for i in range(5)])), k
        assert same_bits(full_y[k], torch.cat([inf.predict(x5[i:i + 1], {n: v[i:i + 1] for n, v in y5.items()})[k] for i in range(5)])), k
        assert not same_bits(full[k], full_y[k])
    cond, cond_y = inf.condition(x5), inf.condition(y=y5)
    assert cond[0].shape == cond_y[1].shape == (5, 256) and not same_bits(cond[0], cond_y[0])
    # a channels_last input gives the same bits
    cl = inf.predict(x5.contiguous(memory_format=torch.channels_last))
    assert all(same_bits(cl[k], full[k]) for k in full)
    assert same_bits(inf.condition(x5.contiguous(memory_format=torch.channels_last))[1], cond[1])

    # segment: the same logits, and masks that are logits >= threshold of its own logits exactly, at 0.5 and at a second threshold
    thr = ref["none"]["masks"].median().item()
    seg, seg2 = inf.segment(x5), inf.segment(x5, threshold=thr)
    assert set(seg) == {"edges", "masks", "edge_mask", "mask_mask"}
    for s, t in ((seg, 0.5), (seg2, thr)):
        for k, mk in (("edges", "edge_mask"), ("masks", "mask_mask")):
            assert same_bits(s[k], full[k]) and s[mk].dtype == torch.bool and s[mk].shape == s[k].shape
            assert torch.equal(s[mk], s[k] >= t), mk
    assert 0.1 < seg2["mask_mask"].float().mean().item() < 0.9, "the threshold should split the logits"

    # the result is eval-mode arithmetic whatever net.training says, and the flag is left alone
    net.train()
    assert all(same_bits(inf.predict(x5)[k], full[k]) for k in full) and net.training
    net.eval()

    # a graph replay == the eager list, bit for bit
    inf.capture()
    assert all(same_bits(inf.predict(x5)[k], full[k]) for k in full)
    assert all(same_bits(inf.predict(x5, y5)[k], full_y[k]) for k in full)
    sg = inf.segment(x5, threshold=thr)
    assert all(torch.equal(sg[k], seg2[k]) for k in seg2)
    assert torch.equal(inf.segment(x5, threshold=thr + 0.25)["mask_mask"], full["masks"] >= thr + 0.25)
    assert same_bits(inf.condition(y=y5)[0], cond_y[0])

    # nothing above wrote to the module
    assert {n: m.training for n, m in net.named_modules()} == flags
    for k, v in net.state_dict().items():
        assert torch.equal(v, state[k]), f"{k} was modified"

    # refresh(): a stale plan keeps what it was built with; refresh() picks a scaled BatchNorm weight up (eager and replayed)
    bn = net.up[0].conv[1].conv[1]
    saved = bn.weight.detach().clone()
    with torch.no_grad():
        bn.weight.mul_(1.5)
    stale = inf.predict(x5)
    assert all(same_bits(stale[k], full[k]) for k in full), "a stale plan must not see the change"
    inf.refresh()
    new = inf.predict(x5)
    assert not same_bits(new["masks"], full["masks"])
    V.set_conv_precision(prec)
    try:
        with torch.no_grad():
            mod = net(x5)
    finally:
        V.set_conv_precision("f32")
    assert rel_err(new["masks"], mod["masks"]) <= 1e-4, "refresh() did not pick up the new BatchNorm weight"
    with torch.no_grad():
        bn.weight.copy_(saved)
    inf.refresh()
    assert all(same_bits(inf.predict(x5)[k], full[k]) for k in full)


def test_error_paths():
    import vae_play_amd as V
    from vae_play_amd import _lib
    net, x, y, _ = _net(16)
    inf = V.FusedFontInference(net, 2)
    E = _lib.VaePlayHipError
    with pytest.raises(E, match=r"\(n, 3, 16, 16\)"):
        inf.predict(torch.zeros((2, 1, 16, 16), device=DEV))
    with pytest.raises(E, match=r"\(n, 3, 16, 16\)"):
        inf.predict(torch.zeros((2, 3, 16, 17), device=DEV))
    with pytest.raises(E, match=r"\(n, 3, 16, 16\)"):
        inf.predict(torch.zeros((0, 3, 16, 16), device=DEV))
    with pytest.raises(E, match="HIP device"):
        inf.predict(torch.zeros((2, 3, 16, 16)))
    with pytest.raises(E, match="fp32"):
        inf.segment(torch.zeros((2, 3, 16, 16), device=DEV, dtype=torch.float64))
    with pytest.raises(E, match=r"\(n, 143\)"):
        inf.predict(x, {"cls": y["cls"]})
    with pytest.raises(E, match=r"\(n, 143\)"):
        inf.predict(x, {"cls": y["cls"][:, :100], "cnt_style": y["cnt_style"]})
    with pytest.raises(E, match=r"\(n, 5\)"):
        inf.condition(y={"cls": y["cls"], "cnt_style": y["cnt_style"][:, :4]})
    with pytest.raises(E, match=r"\(n, 5\)"):
        inf.predict(x, {"cls": y["cls"], "cnt_style": y["cnt_style"][:2]})
    with pytest.raises(E):
        inf.condition()
