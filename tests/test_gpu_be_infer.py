"""Fused segmentation inference on the GPU (csrc/be_infer.hip, vae_play_amd.infer_be.FusedBEInference): the head kernels through the C
ABI against the fp64 oracle of the single block, the whole plan against the fp64 oracle next to the module path in ``.eval()``, and
the properties that need no oracle.  Shapes, seeded parameters and oracle results: tests/be_infer_ref.py (the host emulation of
tests/test_be_infer_cpu.py runs the same cases)."""
import pytest
import torch

from tests import be_infer_ref as R
from tests.guarded import Guards, api, same_bits, tensor_close
from tests.test_gpu_infer import FLOOR
from tests.util import NORTH_STAR_RTOL, record, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
VP_ERR_ARG = -1


def _p(t):
    from ctypes import c_void_p
    return None if t is None else c_void_p(t.data_ptr())


def _pack_heads(lib, case, width):
    """the three stacked parameter blocks of the case's two heads, written by the pack kernels"""
    c1, c2 = width // 4, width // 8
    keep = []

    def dev(t):
        keep.append(t.to(DEV))
        return _p(keep[-1])
    par1 = torch.full((2, lib.vp_be_up_params_floats(width, c1)), float("nan"), device=DEV)
    par2 = torch.full((2, lib.vp_be_up_params_floats(c1, c2)), float("nan"), device=DEV)
    par3 = torch.full((2, lib.vp_be_predictor_params_floats(c2)), float("nan"), device=DEV)
    for k, p in enumerate(case["params"]):
        for prefix, par, ci, cm in (("conv1.", par1, width, c1), ("conv2.", par2, c1, c2)):
            bn = [dev(p[f"{prefix}conv.{j}.conv.1.{n}"]) for j in (0, 1) for n in ("weight", "bias", "running_mean", "running_var")]
            assert lib.vp_be_up_pack_f32(dev(p[prefix + "conv.0.conv.0.weight"]), *bn[:4], dev(p[prefix + "conv.1.conv.0.weight"]), *bn[4:],
                                         1e-5, _p(par[k]), ci, cm, None) == 0
        q = [dev(p[f"predictor.{i}.conv.0.{n}"]) for i in range(3) for n in ("weight", "bias")]
        assert lib.vp_be_predictor_pack_f32(*q, _p(par3[k]), c2, None) == 0
    torch.cuda.synchronize()
    assert not any(torch.isnan(t).any() for t in (par1, par2, par3))
    return par1, par2, par3


class _ByteGuard:
    """a uint8 output between two runs of sentinel bytes"""

    def __init__(self, n):
        self.buf = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device=DEV)
        self.t = self.buf[64:64 + n]
        self.t.fill_(7)

    def check(self):
        assert bool((self.buf[:64] == 0xA5).all()) and bool((self.buf[64 + self.t.numel():] == 0xA5).all()), "mask: written out of bounds"
        assert int(self.t.max()) <= 1, "mask: an element was never written"


# ---- 5. the kernels through the C ABI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", R.SHAPES)
@pytest.mark.parametrize("width", R.WIDTHS)
def test_head_kernels_vs_fp64_oracle(width, h, w):
    """Every supported (cin, cmid) -- (width, width/4) as the first Up block with ONE input for both heads, (width/4, width/8) as the
    second with an input per head -- and the predictor at width/8, heads = 2 and 1, mask and no mask."""
    _lib, _, lib = api()
    case = R.head_case(width, h, w)
    B, c1, c2 = R.BATCH, width // 4, width // 8
    par1, par2, par3 = _pack_heads(lib, case, width)
    x = R.nhwc(case["x"]).to(DEV)
    x2 = torch.stack([R.nhwc(t) for t in case["u1_in"]]).to(DEV)
    x3 = torch.stack([R.nhwc(t.float()) for t in case["u2"]]).to(DEV)
    ref = torch.stack(case["logits"])
    thr = ref.median().item()
    g = Guards()
    y1, y1b = g.out("up1", 2, B, 2 * h, 2 * w, c1), g.out("up1 head 1 alone", 1, B, 2 * h, 2 * w, c1)
    y2, y2b = g.out("up2", 2, B, 4 * h, 4 * w, c2), g.out("up2 head 0 alone", 1, B, 4 * h, 4 * w, c2)
    lg, lgb = g.out("logits", 2, B, 1, 4 * h, 4 * w), g.out("logits head 1 alone", 1, B, 1, 4 * h, 4 * w)
    mask = _ByteGuard(lg.numel())
    _lib.check(lib.vp_be_up_infer_f32(_p(x), 0, _p(par1), _p(y1), 2, B, h, w, width, c1, None), "up1")
    _lib.check(lib.vp_be_up_infer_f32(_p(x), 0, _p(par1[1]), _p(y1b), 1, B, h, w, width, c1, None), "up1 x1")
    _lib.check(lib.vp_be_up_infer_f32(_p(x2), x2[0].numel(), _p(par2), _p(y2), 2, B, 2 * h, 2 * w, c1, c2, None), "up2")
    _lib.check(lib.vp_be_up_infer_f32(_p(x2), 0, _p(par2), _p(y2b), 1, B, 2 * h, 2 * w, c1, c2, None), "up2 x1")
    _lib.check(lib.vp_be_predictor_infer_f32(_p(x3), x3[0].numel(), _p(par3), _p(lg), _p(mask.t), thr, 2, B, 4 * h, 4 * w, c2, None), "pred")
    _lib.check(lib.vp_be_predictor_infer_f32(_p(x3[1]), 0, _p(par3[1]), _p(lgb), None, 0.0, 1, B, 4 * h, 4 * w, c2, None), "pred x1")
    g.check()
    mask.check()
    for k in range(2):
        tag = f"w{width} {h}x{w} head{k}"
        tensor_close(y1[k].permute(0, 3, 1, 2), case["u1"][k], f"up ({width},{c1}) {tag}")
        tensor_close(y2[k].permute(0, 3, 1, 2), case["u2"][k], f"up ({c1},{c2}) {tag}")
        tensor_close(lg[k], case["logits"][k], f"predictor {c2} {tag}")
    assert same_bits(y1b[0], y1[1]) and same_bits(y2b[0], y2[0]) and same_bits(lgb[0], lg[1]), "a head depends on the launch it is in"
    m = mask.t.view(lg.shape).bool().cpu()
    assert torch.equal(m, lg.cpu() >= thr)
    clear = (ref - thr).abs() > 2e-5 * ref.abs().max()
    assert torch.equal(m[clear], (ref >= thr)[clear])


def test_bad_arguments_are_refused_and_launch_nothing():
    _, _, lib = api()
    B, h, w = 1, 4, 4
    x = torch.zeros((2, B, h, w, 32), device=DEV)
    par = torch.zeros((2, 4096), device=DEV)
    y = torch.full((2, B, 2 * h, 2 * w, 8), float("nan"), device=DEV)
    lg = torch.full((2, B, h, w), float("nan"), device=DEV)
    up = lambda *a: lib.vp_be_up_infer_f32(*a, None)            # noqa: E731
    pr = lambda *a: lib.vp_be_predictor_infer_f32(*a, None)     # noqa: E731
    bad_up = [(None, 0, _p(par), _p(y), 2, B, h, w, 32, 8), (_p(x), 0, None, _p(y), 2, B, h, w, 32, 8), (_p(x), 0, _p(par), None, 2, B, h, w, 32, 8),
              (_p(x), 0, _p(par), _p(y), 2, B, h, w, 24, 6), (_p(x), 0, _p(par), _p(y), 2, B, h, w, 32, 4), (_p(x), 0, _p(par), _p(y), 2, B, h, w, 8, 8),
              (_p(x), 0, _p(par), _p(y), 0, B, h, w, 32, 8), (_p(x), 0, _p(par), _p(y), 2, 0, h, w, 32, 8), (_p(x), 0, _p(par), _p(y), 2, B, -1, w, 32, 8),
              (_p(x), 0, _p(par), _p(y), 2, B, h, 0, 32, 8), (_p(x), 2, _p(par), _p(y), 2, B, h, w, 32, 8)]
    for a in bad_up:
        assert up(*a) == VP_ERR_ARG, a
    assert lib.vp_last_error()
    bad_pr = [(None, 0, _p(par), _p(lg), None, 0.0, 2, B, h, w, 8), (_p(x), 0, None, _p(lg), None, 0.0, 2, B, h, w, 8),
              (_p(x), 0, _p(par), None, None, 0.0, 2, B, h, w, 8), (_p(x), 0, _p(par), _p(lg), None, 0.0, 2, B, h, w, 3),
              (_p(x), 0, _p(par), _p(lg), None, 0.0, 2, B, h, w, 16), (_p(x), 0, _p(par), _p(lg), None, 0.0, 0, B, h, w, 8),
              (_p(x), 0, _p(par), _p(lg), None, 0.0, 2, B, 0, w, 8), (_p(x), 0, _p(par), _p(lg), None, 0.0, 2, -3, h, w, 8)]
    for a in bad_pr:
        assert pr(*a) == VP_ERR_ARG, a
    ten = [_p(x)] * 10
    assert lib.vp_be_up_pack_f32(*ten, 1e-5, _p(par), 24, 6, None) == VP_ERR_ARG
    assert lib.vp_be_up_pack_f32(*ten[:9], None, 1e-5, _p(par), 32, 8, None) == VP_ERR_ARG
    assert lib.vp_be_predictor_pack_f32(*ten[:6], _p(par), 5, None) == VP_ERR_ARG
    assert lib.vp_be_predictor_pack_f32(*ten[:6], None, 4, None) == VP_ERR_ARG
    assert lib.vp_be_fold_conv_f32(*ten[:5], 1e-5, _p(par), _p(par), 0, 4, None) == VP_ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(lg).all() and not par.any(), "a refused call wrote"


# ---- the ReLU the gather family's epilogue gained (what lets an aux_convs layer be ONE launch) ----------------------------------
_RELU_SHAPES = [(2, 64, 32, 9, 17, 1), (2, 32, 32, 9, 17, 3), (2, 256, 128, 3, 5, 1), (2, 32, 32, 32, 32, 5)]


@pytest.mark.parametrize("prec,B,Cb,Cs,H,W,ks", [(p, *s) for p in ("f32", "bf16x3") for s in _RELU_SHAPES] + [("f32", 4, 64, 3, 64, 64, 5)])
def test_gather_epilogue_relu_is_the_clamped_plain_result(prec, B, Cb, Cs, H, W, ks):
    """act = relu gives max(acc + bias, 0) of the SAME sum, bit for bit, on every route these shapes take (the k x k kernels the plan
    uses and the 5x5 halo route); at a shape whose none | sigmoid form takes the narrow-output kernel, to the single-op tolerance."""
    _, ops, _ = api()
    g = R.gen(B + Cb + Cs + H + ks)
    x = torch.randn((B, Cb, H, W), generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    wt = (torch.randn((Cs, Cb, ks, ks), generator=g) / (Cb * ks * ks) ** 0.5).to(DEV)
    bias = torch.randn(Cs, generator=g).to(DEV)
    if prec == "f32":
        p0, _ = ops.pack_w(wt, True, False)
        plain = ops.conv_gather(x, p0, bias, ks, 1, ops.ACT_NONE)
        relu = ops.conv_gather(x, p0, bias, ks, 1, ops.ACT_RELU)
    else:
        p0, _ = ops.pack_w_split(wt, True, False)
        xs = ops.split_f32(x)
        plain = ops.conv_gather_bf16x3(xs, x.shape, p0, Cs, bias, ks, 1, ops.ACT_NONE)
        relu = ops.conv_gather_bf16x3(xs, x.shape, p0, Cs, bias, ks, 1, ops.ACT_RELU)
    torch.cuda.synchronize()
    assert 0.2 < (plain > 0).float().mean().item() < 0.8
    want = torch.clamp_min(plain, 0.0)
    if prec == "f32" and Cs == 3:       # the plain form runs on the narrow-output kernel, the relu form on the implicit GEMM: other sum order
        assert rel_err(relu, want) <= 2e-5 and bool((relu >= 0).all())
    else:
        assert torch.equal(relu, want)


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------
NETS = {"be": (R.SHAPES[3], R.SHAPES[4]), "gan": (R.SHAPES[1], R.SHAPES[3])}
_E2E = {}


def _e2e(kind, h, w):
    """the net on the GPU, a seeded feature map and the fp64 oracle's outputs: one evaluation per (net, shape), shared by the precisions"""
    key = (kind, h, w)
    if key not in _E2E:
        net = R.seeded_net(kind)
        x = torch.randn((R.BATCH, 256, h, w), generator=R.gen(40 + h + w))
        _E2E[key] = (net.to(DEV), x, R.oracle_net(net, x))
    return _E2E[key]


@pytest.mark.parametrize("kind,h,w", [(k, *s) for k, shapes in NETS.items() for s in shapes])
@pytest.mark.parametrize("prec", ("f32", "bf16x3"))
def test_end_to_end_vs_fp64_oracle(prec, kind, h, w):
    """tests/test_gpu_infer.py's rule: every output within NORTH_STAR_RTOL of the fp64 oracle, and err_fused <= max(2 err_modules,
    FLOOR[precision]) with err_modules = the same net in .eval() on the GPU with the same weights."""
    import vae_play_amd as V
    net, x, ref = _e2e(kind, h, w)
    xd = x.to(DEV)
    inf = V.FusedBEInference(net, R.BATCH, h, w, precision=prec)
    out = inf.predict(xd)
    out["features"] = inf.features(xd)
    V.set_conv_precision(prec)
    try:
        with torch.no_grad():
            mod = net(xd)
            mod["features"] = (net.aux_convs if kind == "gan" else net.feature_net.aux_convs)(xd)
    finally:
        V.set_conv_precision("f32")
    torch.cuda.synchronize()
    tag = f"{kind} {prec} {h}x{w}"
    fails = []
    for name in ("features", "edges", "masks"):
        assert out[name].shape == ref[name].shape
        ef, em = rel_err(out[name], ref[name]), rel_err(mod[name], ref[name])
        record(f"be infer fused {tag} {name}", ef)
        record(f"be infer modules {tag} {name}", em)
        print(f"{tag} {name}: fused {ef:.3e}  modules {em:.3e}")
        if not ef <= NORTH_STAR_RTOL:
            fails.append(f"{name}: fused {ef:.3e} > {NORTH_STAR_RTOL:.0e}")
        if not ef <= max(2 * em, FLOOR[prec]):
            fails.append(f"{name}: fused {ef:.3e} > max(2 x modules {em:.3e}, floor {FLOOR[prec]:.1e})")
    assert not fails, "; ".join(fails)
    assert net.training is False


# ---- 7. properties that need no oracle -------------------------------------------------------------------------------------------
def _snapshot(inf):
    lists = {w: [(c[0], tuple(getattr(a, "value", a) for a in c[2][:-1])) for plan in inf._plans[w] for c in plan.calls] for w in inf._plans}
    lists["prep"] = [(c[0], tuple(getattr(a, "value", a) for a in c[2][:-1])) for c in inf._prep.calls]
    return lists


@pytest.mark.parametrize("prec", ("f32", "bf16x3"))
def test_properties_without_oracle(prec):
    import vae_play_amd as V
    h, w = R.SHAPES[3]
    net, x5, ref = _e2e("be", h, w)
    x5 = torch.randn((5, 256, h, w), generator=R.gen(77)).to(DEV)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    flags = {n: m.training for n, m in net.named_modules()}
    inf = V.FusedBEInference(net, 2, h, w, precision=prec)
    lists = _snapshot(inf)
    inf.refresh()
    assert _snapshot(inf) == lists, "a second refresh() changed a launch list"

    # a 5-image input through a batch_size 2 plan == its three chunks run separately
    full = inf.predict(x5)
    assert full["edges"].shape == full["masks"].shape == (5, 1, 4 * h, 4 * w)
    parts = [inf.predict(x5[i:i + 2]) for i in (0, 2, 4)]
    for k in ("edges", "masks"):
        assert same_bits(full[k], torch.cat([p[k] for p in parts])), k
    # rows are independent: permuting the batch permutes the outputs
    perm = torch.tensor([3, 0, 4, 2, 1], device=DEV)
    shuffled = inf.predict(x5[perm])
    for k in ("edges", "masks"):
        assert same_bits(shuffled[k], full[k][perm]), f"{k}: a row depends on its batch"
    # a channels_last input takes the list without the transposing copy and gives the same bits
    cl = inf.predict(x5.contiguous(memory_format=torch.channels_last))
    assert all(same_bits(cl[k], full[k]) for k in full)
    f_full = inf.features(x5)
    assert f_full.shape == (5, 32, h, w) and same_bits(inf.features(x5.contiguous(memory_format=torch.channels_last)), f_full)

    # segment: the same logits, and masks that are logits >= threshold of its own logits exactly
    thr = ref["masks"].median().item()
    seg = inf.segment(x5, thr)
    assert set(seg) == {"edges", "masks", "edge_mask", "mask_mask"}
    for k, mk in (("edges", "edge_mask"), ("masks", "mask_mask")):
        assert same_bits(seg[k], full[k]) and seg[mk].dtype == torch.bool and seg[mk].shape == seg[k].shape
        assert torch.equal(seg[mk], seg[k] >= thr), mk
    assert 0.2 < seg["mask_mask"].float().mean().item() < 0.8, "the threshold should split the logits"
    assert torch.equal(inf.segment(x5)["mask_mask"], full["masks"] >= 0.5)

    # the result is eval-mode arithmetic whatever net.training says, and the flag is left alone
    net.train()
    assert all(same_bits(inf.predict(x5)[k], full[k]) for k in full) and net.training
    net.eval()

    # a graph replay == the eager list, bit for bit
    inf.capture()
    g = inf.predict(x5)
    assert all(same_bits(g[k], full[k]) for k in full)
    sg = inf.segment(x5, thr)
    assert all(torch.equal(sg[k], seg[k]) for k in seg)
    sg2 = inf.segment(x5, thr + 1.0)                              # (a new threshold is captured again)
    assert torch.equal(sg2["mask_mask"], full["masks"] >= thr + 1.0)
    assert same_bits(inf.features(x5), f_full)

    # nothing above wrote to the module
    assert {n: m.training for n, m in net.named_modules()} == flags
    for k, v in net.state_dict().items():
        assert torch.equal(v, state[k]), f"{k} was modified"

    # refresh(): a stale plan keeps what it was built with; refresh() picks a changed BatchNorm buffer up (eager and replayed)
    bn = net.mask_net.conv1.conv[1].conv[1]
    saved = bn.running_var.clone()
    with torch.no_grad():
        bn.running_var.mul_(3.0)
    stale = inf.predict(x5)
    assert all(same_bits(stale[k], full[k]) for k in full), "a stale plan must not see the change"
    inf.refresh()
    new = inf.predict(x5)
    assert not same_bits(new["masks"], full["masks"]) and same_bits(new["edges"], full["edges"])
    with torch.no_grad():
        mod = net(x5)
    assert rel_err(new["masks"], mod["masks"]) <= 1e-4, "refresh() did not pick up the new running statistics"
    with torch.no_grad():
        bn.running_var.copy_(saved)
    inf.refresh()
    back = inf.predict(x5)
    assert all(same_bits(back[k], full[k]) for k in full)


def test_error_paths():
    import vae_play_amd as V
    from vae_play_amd import _lib
    net, _, _ = _e2e("be", *R.SHAPES[3])
    h, w = R.SHAPES[3]
    inf = V.FusedBEInference(net, 2, h, w)
    with pytest.raises(_lib.VaePlayHipError, match="shape"):
        inf.predict(torch.zeros((2, 128, h, w), device=DEV))
    with pytest.raises(_lib.VaePlayHipError, match="shape"):
        inf.predict(torch.zeros((2, 256, h, w + 1), device=DEV))
    with pytest.raises(_lib.VaePlayHipError, match="HIP device"):
        inf.predict(torch.zeros((2, 256, h, w)))
    with pytest.raises(_lib.VaePlayHipError, match="fp32"):
        inf.segment(torch.zeros((2, 256, h, w), device=DEV, dtype=torch.float64))
