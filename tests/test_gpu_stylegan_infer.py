"""Fused Style-GAN inference on the GPU (csrc/stylegan_infer.hip, vae_play_amd.infer_stylegan.FusedStyleGanInference): the new kernels
through the C ABI against fp64, the whole plan against the fp64 restatements next to the modules under ``torch.no_grad()``, and the
properties that need no oracle.  Cases, seeded nets and fp64 results: tests/stylegan_infer_ref.py."""
from ctypes import c_void_p

import pytest
import torch
import torch.nn.functional as F

from tests import stylegan_infer_ref as R
from tests.guarded import Guards, api, same_bits, tensor_close
from tests.test_gpu_infer import FLOOR
from tests.util import NORTH_STAR_RTOL, record, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
VP_ERR_ARG, VP_ERR_WORKSPACE = -1, -3


def _p(t, offset_floats=0):
    return None if t is None else c_void_p(t.data_ptr() + 4 * offset_floats)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- 1. vp_scse2_fwd_f32 through the C ABI ---------------------------------------------------------------------------------------------
def _scse_dev(sd, pre):
    """one block's six parameters on the device, in the entry's order (the 1x1 weights as they are stored)"""
    return [sd[f"{pre}.{k}"].contiguous().to(DEV) for k in R.SCSE_KEYS]


def _scse2(lib, x, pa, pb, y, ys, B, HW, C, hidden, relu, ws, nbytes):
    return lib.vp_scse2_fwd_f32(_p(x), *map(_p, pa), *map(_p, pb), _p(y), _p(ys), B, HW, C, hidden, relu, _p(ws), nbytes, None)


@pytest.mark.parametrize("case", range(len(R.SCSE2_CASES)))
def test_scse2_kernel_vs_fp64(case):
    """relu 0 and 1, with the bf16 planes where C % 8 == 0: fp64 scse(scse(x)), guards, NaN-filled outputs, exact zeros for the all-zero
    image, planes that recombine to y within 2^-16, the same bits from a second run"""
    _lib, _, lib = api()
    B, C, H, W, red = R.SCSE2_CASES[case]
    hidden, HW = C // red, H * W
    x, sd, ref = R.scse2_case(case)
    xd = _nhwc(x).to(DEV)
    pa, pb = _scse_dev(sd, "a"), _scse_dev(sd, "b")
    nbytes = lib.vp_scse2_workspace_bytes(B, HW, C, hidden)
    assert nbytes > 0 and nbytes % 4 == 0
    for relu in (0, 1):
        for planes in ((False, True) if C % 8 == 0 else (False,)):
            g = Guards()
            y, y2 = g.out("y", B, H, W, C), g.out("y again", B, H, W, C)
            ws, _ = g.ws("ws", nbytes)
            ys = g.planes("y planes", y.numel()) if planes else None
            _lib.check(_scse2(lib, xd, pa, pb, y, ys, B, HW, C, hidden, relu, ws, nbytes), "vp_scse2_fwd_f32")
            _lib.check(_scse2(lib, xd, pa, pb, y2, None, B, HW, C, hidden, relu, ws, nbytes), "vp_scse2_fwd_f32")
            g.check()
            tensor_close(y.permute(0, 3, 1, 2), ref[relu], f"scse2 case {case} {R.SCSE2_CASES[case]} relu {relu} planes {planes}")
            assert same_bits(y, y2), "two runs differ"
            if B > 1:
                assert bool((y[0] == 0).all()), "an all-zero image must give exact zeros"
            if relu:
                assert bool((y >= 0).all())
            if planes:
                hi_lo = ys.view(torch.bfloat16).float().view(2, -1)
                assert not torch.isnan(hi_lo).any(), "a plane element was never written"
                back = (hi_lo[0] + hi_lo[1]).view(y.shape)
                assert bool(((back - y).abs() <= 2.0 ** -16 * y.abs()).all()), "the planes do not recombine to y"


def test_scse2_refusals_write_nothing():
    _, _, lib = api()
    B, C, H, W, hidden = 2, 32, 4, 4, 8
    HW = H * W
    x = torch.zeros((B, H, W, C), device=DEV)
    par = [torch.zeros(n, device=DEV) for n in (hidden * C, hidden, C * hidden, C, C, 1)]
    y = torch.full((B, H, W, C), float("nan"), device=DEV)
    ys = torch.full((2, B * HW * C), 0x7FC0, dtype=torch.int16, device=DEV)
    big = torch.zeros(B * HW * 1024 + 4, device=DEV)
    nbytes = lib.vp_scse2_workspace_bytes(B, HW, C, hidden)
    ws = torch.full((nbytes // 4 + 4,), float("nan"), device=DEV)
    good = [_p(x)] + [_p(t) for t in par] * 2 + [_p(y), _p(ys), B, HW, C, hidden, 1, _p(ws), nbytes]
    call = lambda a: lib.vp_scse2_fwd_f32(*a, None)       # noqa: E731

    def bad(i, v, **more):
        a = list(good)
        a[i] = v
        for k, w in more.items():
            a[int(k[1:])] = w
        return a
    # null x, null parameters of either block, null y, null workspace; B, HW, C = 0; hidden 0 and > C; C past both ranges
    arg = [bad(0, None), bad(1, None), bad(6, None), bad(7, None), bad(12, None), bad(13, None), bad(20, None), bad(15, 0), bad(16, 0),
           bad(17, 0), bad(18, 0), bad(18, C + 1), bad(17, 1028), bad(17, 258, _18=8),
           # planes with C % 8 != 0, misaligned planes, a misaligned tensor with planes asked for
           bad(17, 12, _18=3), bad(14, c_void_p(ys.data_ptr() + 2)), bad(0, _p(x, 1)),
           # C = 1024 needs the 16-byte path: a misaligned x or workspace is refused
           bad(0, _p(big, 1), _17=1024, _18=64, _14=None, _13=_p(big), _21=1 << 30), bad(20, _p(big, 1), _17=1024, _18=64, _14=None, _21=1 << 30)]
    for a in arg:
        assert call(a) == VP_ERR_ARG, a
    assert lib.vp_last_error()
    for short in (0, 4, nbytes - 4):
        assert call(bad(21, short)) == VP_ERR_WORKSPACE, short
    assert b"workspace" in lib.vp_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(ws).all() and bool((ys == 0x7FC0).all()), "a refused call wrote"
    # and the same arguments, untouched, are taken
    assert call(good) == 0
    torch.cuda.synchronize()
    assert bool((y == 0).all())


# ---- 2. vp_cat2_nhwc_f32 and vp_sg_out_tanh_f32 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,Ca,Cb", [(2, 35, 3, 1), (3, 64, 3, 3)])
def test_cat2_all_layouts_equal_torch(B, HW, Ca, Cb):
    _lib, _, lib = api()
    g0 = R.gen(31 + HW)
    a, b = torch.randn((B, Ca, HW), generator=g0), torch.randn((B, Cb, HW), generator=g0)      # NCHW with H*W flattened
    want = torch.cat([a, b], dim=1).permute(0, 2, 1).contiguous()                               # [B][HW][Ca + Cb]
    src = {0: lambda t: t.contiguous().to(DEV), 1: lambda t: t.permute(0, 2, 1).contiguous().to(DEV)}
    for fa in (0, 1):
        for fb in (0, 1):
            g = Guards()
            out = g.out(f"cat {fa}{fb}", B, HW, Ca + Cb)
            ad, bd = src[fa](a), src[fb](b)
            _lib.check(lib.vp_cat2_nhwc_f32(_p(ad), fa, _p(bd), fb, _p(out), B, HW, Ca, Cb, None), "vp_cat2_nhwc_f32")
            g.check()
            assert torch.equal(out.cpu(), want), (fa, fb)
    x = torch.zeros(8, device=DEV)
    for a_ in ((None, 0, _p(x), 0, _p(x), 1, 1, 1, 1), (_p(x), 0, None, 0, _p(x), 1, 1, 1, 1), (_p(x), 0, _p(x), 0, None, 1, 1, 1, 1),
               (_p(x), 0, _p(x), 0, _p(x), 0, 1, 1, 1), (_p(x), 0, _p(x), 0, _p(x), 1, 0, 1, 1), (_p(x), 0, _p(x), 0, _p(x), 1, 1, 0, 1),
               (_p(x), 0, _p(x), 0, _p(x), 1, 1, 1, -1)):
        assert lib.vp_cat2_nhwc_f32(*a_, None) == VP_ERR_ARG, a_


@pytest.mark.parametrize("B,H,W,C", [(2, 8, 8, 32), (2, 5, 7, 64), (1, 3, 4, 12)])      # 8, 16 and 4 lanes per pixel
def test_sg_out_tanh_vs_fp64(B, H, W, C):
    """tanh(conv2d) in fp64; the three output channels carry distinct biases, so a wrong NCHW plane order cannot pass"""
    _lib, _, lib = api()
    g0 = R.gen(500 + H)
    x = torch.randn((B, H, W, C), generator=g0)
    w = (torch.rand((3, C, 3, 3), generator=g0) * 2 - 1) * (3.0 / (9 * C)) ** 0.5
    bias = torch.tensor([-0.9, 0.1, 0.8])
    with torch.no_grad():
        ref = torch.tanh(F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), bias.double(), padding=1))
    assert (ref[:, 0].mean() < ref[:, 1].mean() < ref[:, 2].mean())
    n_par = lib.vp_sg_out_params_floats(C)
    g = Guards()
    par, out = g.out("params", n_par), g.out("out", B, 3, H, W)
    wd, bd, xd = w.to(DEV), bias.to(DEV), x.to(DEV)
    _lib.check(lib.vp_sg_out_pack_f32(_p(wd), _p(bd), _p(par), C, None), "pack")
    _lib.check(lib.vp_sg_out_tanh_f32(_p(xd), _p(par), _p(out), B, H, W, C, None), "vp_sg_out_tanh_f32")
    g.check()
    assert torch.equal(par[:27 * C].view(3, 9, C).cpu(), w.permute(0, 2, 3, 1).reshape(3, 9, C)) and torch.equal(par[27 * C:27 * C + 3].cpu(), bias)
    tensor_close(out, ref, f"sg_out_tanh {H}x{W} C{C}")
    # refused: null and misaligned pointers, channel counts off the grid, empty sizes
    nan = torch.full((B, 3, H, W), float("nan"), device=DEV)
    for a in ((None, _p(par), _p(nan), B, H, W, C), (_p(xd), None, _p(nan), B, H, W, C), (_p(xd), _p(par), None, B, H, W, C),
              (_p(xd, 1), _p(par), _p(nan), B, H, W, C), (_p(xd), _p(par), _p(nan), B, H, W, 6), (_p(xd), _p(par), _p(nan), B, H, W, 260),
              (_p(xd), _p(par), _p(nan), 0, H, W, C), (_p(xd), _p(par), _p(nan), B, 0, W, C)):
        assert lib.vp_sg_out_tanh_f32(*a, None) == VP_ERR_ARG, a
    assert lib.vp_sg_out_pack_f32(_p(wd), None, _p(par), C, None) == VP_ERR_ARG
    assert lib.vp_sg_out_pack_f32(_p(wd), _p(bd), _p(par), 6, None) == VP_ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(nan).all(), "a refused call wrote"


# ---- 3. the whole plan -----------------------------------------------------------------------------------------------------------------
_DEV = {}


def _case(S):
    if S not in _DEV:
        import copy
        nets, inp, ref = R.net_case(S)
        _DEV[S] = (tuple(copy.deepcopy(n).to(DEV) for n in nets), {k: v.to(DEV) for k, v in inp.items()}, ref)
    return _DEV[S]


def _modules(nets, inp, prec):
    """every output through the autograd modules under torch.no_grad(), in the plan's convolution arithmetic"""
    import vae_play_amd as V
    G, E, D = nets
    B = inp["z"].shape[0]
    V.set_conv_precision(prec)
    try:
        with torch.no_grad():
            out = {"generate": G(inp["x_content"], inp["z"], inp["labels"])}
            for c in (0, 1):
                out[f"generate{c}"] = G(inp["x_content"], inp["z"], torch.full((B,), float(c), device=DEV))
            out["mu"], out["logvar"] = E(inp["x_style"])
            out["stylize"] = G(inp["x_content"], out["mu"] + inp["eps"] * torch.exp(out["logvar"] / 2), inp["labels"])
            out["adv"], out["aux"] = D(inp["x"], inp["x_content"], None)
    finally:
        V.set_conv_precision("f32")
    return out


@pytest.mark.parametrize("S", R.SIZES)
@pytest.mark.parametrize("prec", ("f32", "bf16x3"))
def test_whole_plan_vs_fp64_oracle(prec, S):
    """tests/test_gpu_infer.py's rule: every output within NORTH_STAR_RTOL of the fp64 oracle, and err_fused <= max(2 err_modules,
    FLOOR[precision]) with err_modules = the same nets on the GPU with the same weights.  The int-label lists (labels = 0, labels = 1)
    against the oracle with every label 0 / 1."""
    import vae_play_amd as V
    nets, inp, ref = _case(S)
    inf = V.FusedStyleGanInference(*nets, batch_size=R.BATCH, precision=prec)
    out = {"generate": inf.generate(inp["x_content"], inp["z"], inp["labels"]),
           "generate0": inf.generate(inp["x_content"], inp["z"], 0), "generate1": inf.generate(inp["x_content"], inp["z"], 1),
           "stylize": inf.stylize(inp["x_content"], inp["x_style"], inp["labels"], eps=inp["eps"])}
    out["mu"], out["logvar"] = inf.encode_style(inp["x_style"])
    out["adv"], out["aux"] = inf.discriminate(inp["x"], inp["x_content"])
    mod = _modules(nets, inp, prec)
    torch.cuda.synchronize()
    fails = []
    for name in ("generate", "generate0", "generate1", "stylize", "mu", "logvar", "adv", "aux"):
        assert out[name].shape == ref[name].shape, name
        ef, em = rel_err(out[name], ref[name]), rel_err(mod[name], ref[name])
        record(f"stylegan infer fused {prec} S{S} {name}", ef)
        record(f"stylegan infer modules {prec} S{S} {name}", em)
        print(f"{prec} S{S} {name}: fused {ef:.3e}  modules {em:.3e}")
        if not ef <= NORTH_STAR_RTOL:
            fails.append(f"{name}: fused {ef:.3e} > {NORTH_STAR_RTOL:.0e}")
        if not ef <= max(2 * em, FLOOR[prec]):
            fails.append(f"{name}: fused {ef:.3e} > max(2 x modules {em:.3e}, floor {FLOOR[prec]:.1e})")
    assert not fails, "; ".join(fails)
    assert rel_err(out["generate0"], ref["generate1"]) > 1e-2, "labels 0 and 1 must give different images"


# ---- 4. properties that need no oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ("f32", "bf16x3"))
def test_properties_without_oracle(prec):
    import vae_play_amd as V
    S = 32
    nets, _, _ = _case(S)
    G, E, D = nets
    g0 = R.gen(88)
    xc, xs, x = (torch.rand((5, 3, S, S), generator=g0).to(DEV) for _ in range(3))
    z, eps = torch.randn((5, R.Z), generator=g0).to(DEV), torch.randn((5, R.Z), generator=g0).to(DEV)
    lab = torch.tensor([0, 1, 1, 0, 1])                       # int64, as the reference passes it
    state = [{k: v.detach().clone() for k, v in n.state_dict().items()} for n in nets]
    flags = [{k: m.training for k, m in n.named_modules()} for n in nets]
    inf = V.FusedStyleGanInference(G, E, D, batch_size=3, precision=prec)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)        # noqa: E731

    def run_all():
        r = {"gen": inf.generate(xc, z, lab), "gen1": inf.generate(xc, z, 1), "sty": inf.stylize(xc, xs, lab, eps=eps),
             "sty_mu": inf.stylize(xc, xs, lab), "sty0": inf.stylize(xc, xs, 0)}
        r["mu"], r["logvar"] = inf.encode_style(xs)
        r["adv"], r["aux"] = inf.discriminate(x, xc)
        return r
    full = run_all()
    assert full["gen"].shape == (5, 3, S, S) and full["mu"].shape == (5, R.Z) and full["adv"].shape == (5, 1) and full["aux"].shape == (5, R.CLASSES)

    # n = 5 through a batch_size 3 plan == the five images one at a time
    one = lambda t, i: t[i:i + 1]                                          # noqa: E731
    assert same_bits(full["gen"], torch.cat([inf.generate(one(xc, i), one(z, i), one(lab, i)) for i in range(5)]))
    assert same_bits(full["gen1"], torch.cat([inf.generate(one(xc, i), one(z, i), 1) for i in range(5)]))
    assert same_bits(full["sty"], torch.cat([inf.stylize(one(xc, i), one(xs, i), one(lab, i), eps=one(eps, i)) for i in range(5)]))
    assert same_bits(full["mu"], torch.cat([inf.encode_style(one(xs, i))[0] for i in range(5)]))
    assert same_bits(full["aux"], torch.cat([inf.discriminate(one(x, i), one(xc, i))[1] for i in range(5)]))
    # a channels_last input gives the same bits
    assert same_bits(inf.generate(cl(xc), z, lab), full["gen"]) and same_bits(inf.generate(cl(xc), z, 1), full["gen1"])
    assert same_bits(inf.stylize(cl(xc), cl(xs), lab, eps=eps), full["sty"]) and same_bits(inf.stylize(cl(xc), xs, lab, eps=eps), full["sty"])
    assert same_bits(inf.encode_style(cl(xs))[1], full["logvar"])
    assert same_bits(inf.discriminate(cl(x), cl(xc))[0], full["adv"]) and same_bits(inf.discriminate(x, cl(xc))[1], full["aux"])
    # stylize without eps is generate of encode_style's mu; a float label is that label for every image
    assert same_bits(full["sty_mu"], inf.generate(xc, full["mu"], lab))
    assert same_bits(inf.generate(xc, z, 1.0), inf.generate(xc, z, torch.ones(5)))
    # the two classes differ, in the blended and in the single-class lists
    assert rel_err(inf.generate(xc, z, 0), full["gen1"]) > 1e-2 and rel_err(inf.generate(xc, z, 0.0), inf.generate(xc, z, 1.0)) > 1e-2
    assert rel_err(full["gen1"], inf.generate(xc, z, 1.0)) <= 1e-4, "the single-class list and the blended list disagree at label 1"

    # a graph replay == the eager list, bit for bit
    inf.capture()
    again = run_all()
    for k in full:
        assert same_bits(again[k], full[k]), k
    assert same_bits(inf.generate(cl(xc), z, lab), full["gen"])

    # nothing above wrote to the modules
    assert [{k: m.training for k, m in n.named_modules()} for n in nets] == flags
    for n, st in zip(nets, state):
        for k, v in n.state_dict().items():
            assert torch.equal(v, st[k]), f"{k} was modified"

    # refresh(): a stale plan keeps what it was built with; refresh() picks a scaled weight up (eager and replayed)
    w = G.up2.cat_convs[0].conv[0].weight
    saved = w.detach().clone()
    try:
        with torch.no_grad():
            w.mul_(1.5)
        assert same_bits(inf.generate(xc, z, lab), full["gen"]), "a stale plan must not see the change"
        inf.refresh()
        new = inf.generate(xc, z, lab)
        assert not same_bits(new, full["gen"])
        V.set_conv_precision(prec)
        try:
            with torch.no_grad():
                mod = G(xc, z, lab)
        finally:
            V.set_conv_precision("f32")
        assert rel_err(new, mod) <= 1e-4, "refresh() did not pick up the new weight"
    finally:
        with torch.no_grad():
            w.copy_(saved)
    inf.refresh()
    assert same_bits(inf.generate(xc, z, lab), full["gen"])


def test_error_paths():
    import vae_play_amd as V
    from vae_play_amd import _lib
    nets, inp, _ = _case(32)
    inf = V.FusedStyleGanInference(*nets, batch_size=2, precision="f32")
    E = _lib.VaePlayHipError
    xc, z, lab = inp["x_content"], inp["z"], inp["labels"]
    img = r"\(n, 3, 32, 32\)"
    with pytest.raises(E, match=img):
        inf.generate(torch.zeros((3, 1, 32, 32), device=DEV), z, lab)
    with pytest.raises(E, match=img):
        inf.generate(torch.zeros((0, 3, 32, 32), device=DEV), z, lab)
    with pytest.raises(E, match=img):
        inf.encode_style(torch.zeros((3, 3, 32, 33), device=DEV))
    with pytest.raises(E, match=img):
        inf.discriminate(xc, xc[:2])
    with pytest.raises(E, match=img):
        inf.stylize(xc, xc[:1], lab)
    with pytest.raises(E, match="HIP device"):
        inf.generate(xc.cpu(), z, lab)
    with pytest.raises(E, match="fp32"):
        inf.generate(xc.double(), z, lab)
    with pytest.raises(E, match=r"\(n, 8\)"):
        inf.generate(xc, z[:, :4], lab)
    with pytest.raises(E, match=r"\(n, 8\)"):
        inf.generate(xc, z[:2], lab)
    with pytest.raises(E, match=r"\(n, 8\)"):
        inf.stylize(xc, xc, lab, eps=z[:2])
    with pytest.raises(E, match=r"\(n,\)"):
        inf.generate(xc, z, lab[:2])
    with pytest.raises(E, match="0 or 1"):
        inf.generate(xc, z, 2)
    only_g = V.FusedStyleGanInference(nets[0], batch_size=2, precision="f32")
    for call in (lambda: only_g.encode_style(xc), lambda: only_g.stylize(xc, xc, 0), lambda: only_g.discriminate(xc, xc)):
        with pytest.raises(E, match="built without one"):
            call()
    assert only_g.generate(xc, z, lab).shape == (3, 3, 32, 32)
