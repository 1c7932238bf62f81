"""Segmentation evaluation on the GPU (csrc/seg_eval.hip, vae_play_amd.seg_eval, FusedBEInference.evaluate,
FusedFontInference.evaluate) against the float64 restatement (tests/seg_eval_ref.py, which tests/test_seg_eval_cpu.py pins): the integer
counts EQUAL, the sums and terms within OP_RTOL -- the project's bar for sums of non-negative terms (targets lie in [0, 1]) -- and two
runs bit-equal.  Direct calls keep outputs and workspace between sentinel guards."""
import copy
import functools
from ctypes import c_void_p

import pytest
import torch
import torch.nn.functional as F

from tests import be_infer_ref as NB
from tests import font_infer_ref as NF
from tests import seg_eval_ref as R
from tests.guarded import Guards, api, same_bits, scalar_close, tensor_close
from tests.util import OP_RTOL, load_golden, t as as_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
# the kernel's tile: SE_TH rows x SE_TW columns of one plane per workgroup (csrc/seg_eval.hip).  One row past the row edge and one column
# past the column edge -- 513 columns take the scalar loads, 516 the 16-byte ones -- so a halo crosses both kinds of tile border
SE_TH, SE_TW = 32, 512
EDGE_SHAPES = ((1, 2, SE_TH + 1, SE_TW + 1), (1, 1, SE_TH + 1, SE_TW + 4))
TOLS = (0, 1, 3)
VP_ERR_ARG, VP_ERR_WORKSPACE = -1, -3


def _place(v, layout):
    """(heads, B, 1, H, W) on the device as (tensor that owns the memory, address of head 0, head stride in floats)"""
    heads, per_head = v.shape[0], v[0].numel()
    if layout == "plain":
        d = v.contiguous().to(DEV)
        assert d.data_ptr() % 16 == 0
        return d, d.data_ptr(), per_head
    if layout == "offset":               # one float past a 16-byte boundary
        d = torch.empty(v.numel() + 4, device=DEV)
        d[1:1 + v.numel()].copy_(v.reshape(-1))
        assert (d.data_ptr() + 4) % 16 == 4
        return d, d.data_ptr() + 4, per_head
    stride = per_head + 12               # "strided": head planes further apart than B * H * W, the gap NaN
    d = torch.full((heads, stride), float("nan"), device=DEV)
    d[:, :per_head].copy_(v.reshape(heads, -1))
    return d, d.data_ptr(), stride


def _call(x, t, tol, layout="plain", threshold=0.5, target_threshold=0.5, bce_weight=0.5, smooth=1.0, ws_bytes=None, expect=0):
    _lib, ops, lib = api()
    x5, t5 = (x if x.dim() == 5 else x[None]), (t if t.dim() == 5 else t[None])
    heads, B, _, H, W = x5.shape
    keep_x, xp, xs = _place(x5, layout)
    keep_t, tp, ts = _place(t5, layout)
    G = Guards(DEV)
    if torch.isfinite(x5).all():
        sums, terms = G.out("sums", heads * B, 4), G.out("terms", heads * B, 3)
    else:                                # NaN is then a legitimate result: guarded at both ends, not checked for unwritten elements
        sums, terms = G.ws("sums", heads * B * 16)[0].view(heads * B, 4), G.ws("terms", heads * B * 12)[0].view(heads * B, 3)
    counts = G.out("counts", heads * B, 6)
    need = lib.vp_seg_eval_workspace_bytes(heads, B, H, W, max(0, min(tol, 4)))
    assert need > 0 and need % 8 == 0
    ws, nbytes = G.ws("ws", need if ws_bytes is None else ws_bytes)
    rc = lib.vp_seg_eval_f32(c_void_p(xp), xs, c_void_p(tp), ts, ops._p(sums), ops._p(terms), ops._p(counts), heads, B, H, W, threshold,
                             target_threshold, bce_weight, smooth, tol, ops._p(ws), nbytes, None)
    assert rc == expect, (rc, lib.vp_last_error())
    if expect != 0:
        torch.cuda.synchronize()
        assert torch.isnan(sums).all() and torch.isnan(terms).all() and torch.isnan(counts).all(), "a refused call wrote"
        return None
    G.check()
    return {"sums": sums.cpu(), "terms": terms.cpu(), "counts": counts.view(torch.int32).cpu()}


def _same_result(a, b):
    return same_bits(a["sums"], b["sums"]) and same_bits(a["terms"], b["terms"]) and torch.equal(a["counts"], b["counts"])


def _against(got, ref, what):
    assert torch.equal(got["counts"].long(), ref["counts"]), f"{what}: counts {got['counts'].tolist()} vs {ref['counts'].tolist()}"
    fin = torch.isfinite(ref["sums"])
    if not fin.all():                    # non-finite logits: non-finite results in the same places, the others held as usual
        assert torch.equal(torch.isfinite(got["sums"]), fin) and torch.equal(torch.isfinite(got["terms"]), torch.isfinite(ref["terms"])), what
        scalar_close(got["sums"][fin], ref["sums"][fin], f"seg eval {what} sums")
        return
    scalar_close(got["sums"], ref["sums"], f"seg eval {what} sums")
    tensor_close(got["terms"], ref["terms"], f"seg eval {what} terms")


@functools.lru_cache(maxsize=None)
def _case(family, shape, tol):
    x, t = R.case(family, shape)
    return x, t, R.reference(x, t, tol=tol)


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("shape", R.SHAPES + EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_kernel_vs_restatement(family, shape, tol):
    x, t, ref = _case(family, shape, tol)
    first = _call(x, t, tol)
    _against(first, ref, f"{family} {shape} tol {tol}")
    assert _same_result(first, _call(x, t, tol)), "two runs differ"
    for layout in ("offset", "strided"):
        _against(_call(x, t, tol, layout), ref, f"{family} {shape} tol {tol} {layout}")


def test_explicit_border_cases():
    """one bit of P and one of T each, a window's width apart only through a row wrap, the next image or the other head"""
    for name, (x, t, tol) in R.explicit_cases().items():
        for layout in ("plain", "offset"):
            _against(_call(x, t, tol, layout), R.reference(x, t, tol=tol), f"explicit {name} {layout}")
    x, t = R.case("sparse", (1, 1, 12, 20))
    for tol in (2, 4):
        _against(_call(x, t, tol), R.reference(x, t, tol=tol), f"sparse tol {tol}")


def test_other_settings():
    x, t = R.case("ring", (2, 3, 12, 20))
    t = t * torch.rand(t.shape, generator=torch.Generator().manual_seed(9))          # soft targets in [0, 1]
    kw = dict(threshold=-0.25, target_threshold=0.3, bce_weight=0.7, smooth=2.5)
    _against(_call(x, t, 1, **kw), R.reference(x, t, tol=1, **kw), "settings")


def test_special_values():
    _, ops, _ = api()
    x, t = R.case("ring", (1, 4, 12, 20))
    x, t = x.clone(), t.clone()
    x[0, 0, 0, 2, 3:9] = 0.5                                   # exactly the threshold: predicted
    x[0, 0, 0, 0, 0], x[0, 0, 0, 11, 19], x[0, 0, 0, 6, 1] = float("inf"), float("-inf"), float("inf")     # sigmoid stays finite
    t[0, 0, 0, 0, 0], t[0, 0, 0, 11, 19], t[0, 0, 0, 6, 1] = 1.0, 0.0, 0.0
    x[0, 1, 0, 5, 7], t[0, 1, 0, 5, 7] = float("nan"), 1.0
    t[0, 2] = 0.0                                               # an all-zero target
    x[0, 3] = x[0, 3].abs() + 1.0                               # all-true predictions
    for tol in (0, 1):
        got, ref = _call(x, t, tol), R.reference(x, t, tol=tol)
        assert torch.equal(got["counts"].long(), ref["counts"]), (got["counts"], ref["counts"])
        assert got["counts"][:, 5].tolist() == [3, 1, 0, 0]
        assert got["counts"][0, 0] >= 6 and got["counts"][3, 0] == 240 and got["counts"][2, 1] == 0 and got["counts"][2, 3] == 0
        # non-finite exactly where torch's float64 sums are
        x64, t64 = x.double().reshape(4, -1), t.double().reshape(4, -1)
        p = torch.sigmoid(x64)
        want = torch.stack([F.binary_cross_entropy_with_logits(x64, t64, reduction="none").sum(1), (p * t64).sum(1), p.sum(1), t64.sum(1)], 1)
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(got["sums"]), fin) and torch.equal(fin, torch.isfinite(ref["sums"])), (got["sums"], want)
        assert fin.tolist() == [[False, True, True, True], [False, False, False, True], [True] * 4, [True] * 4]
        scalar_close(got["sums"][fin], want[fin], f"special sums tol {tol}")
        assert torch.equal(torch.isfinite(got["terms"]), torch.isfinite(ref["terms"]))
        assert torch.isfinite(got["terms"][0, 1]) and not torch.isfinite(got["terms"][0, 2])
        scalar_close(got["terms"][0, 1], ref["terms"][0, 1], f"special dice tol {tol}")
        tensor_close(got["terms"][2:], ref["terms"][2:], f"special terms tol {tol}")


def test_refused_calls_launch_nothing():
    x, t = R.case("sparse", (1, 2, 5, 7))
    for tol in (-1, 5):
        _call(x, t, tol, expect=VP_ERR_ARG)
    _call(x, t, 0, threshold=float("nan"), expect=VP_ERR_ARG)
    _call(x, t, 1, ws_bytes=64, expect=VP_ERR_WORKSPACE)           # two images need two partials of 64 bytes
    _, _, lib = api()
    assert lib.vp_seg_eval_workspace_bytes(1, 1, 4097, 4096, 0) == 0 and lib.vp_seg_eval_workspace_bytes(1, 1, 4, 4, 5) == 0


def test_consistent_with_the_training_loss():
    """the mean over the images of the per-image loss is ops.be_loss_fwd's scalar on the same tensors"""
    _, ops, _ = api()
    import vae_play_amd as V
    for family, shape in (("ring", (1, 3, 12, 20)), ("sparse", (1, 2, 64, 64)), ("ring", (1, 1, 33, 130))):
        x, t = R.case(family, shape)
        xd, td = x[0].to(DEV), t[0].to(DEV)
        out = V.segmentation_metrics(xd, td, bce_weight=0.5, smooth=1.0)
        loss, sums = ops.be_loss_fwd(xd, td, 0.5, 1.0)
        torch.cuda.synchronize()
        scalar_close(out["terms"][:, 2].double().mean(), loss.double().cpu(), f"be_loss {family} {shape}")
        scalar_close(out["sums"], sums.double().cpu().reshape(-1, 4), f"be_loss sums {family} {shape}")


def test_golden_reference_loss():
    import vae_play_amd as V
    g = load_golden("seg_eval")
    for k in range(int(g["n"])):
        x, t = as_tensor(g[f"c{k}/logits"]).to(DEV), as_tensor(g[f"c{k}/targets"]).to(DEV)
        out = V.segmentation_metrics(x, t)
        assert out["sums"].shape == (x.shape[0], 4) and out["terms"].shape == (x.shape[0], 3) and out["counts"].shape == (x.shape[0], 6)
        assert out["counts"].dtype == torch.int32 and out["sums"].is_cuda
        scalar_close(out["terms"][:, 2].double().mean(), float(g[f"c{k}/loss64"]), f"golden loss case {k}")


def test_free_function_on_views_and_tolerances():
    """segmentation_metrics on tensors whose storage offset is odd (a slice of a larger batch) at every tolerance"""
    import vae_play_amd as V
    x, t = R.case("ring", (1, 4, 33, 130))
    xd, td = x[0].to(DEV), t[0].to(DEV)
    for tol in range(5):
        got = V.segmentation_metrics(xd[1:], td[1:], tolerance=tol)
        ref = R.reference(x[0, 1:], t[0, 1:], tol=tol)
        _against({k: v.cpu() for k, v in got.items()}, ref, f"free function tol {tol}")
    s = V.summarize(got)
    c = ref["counts"].sum(0).double()
    assert s["boundary_precision"]["micro"] == (c[3] / c[0]).item() and s["loss"]["macro"] == pytest.approx(ref["terms"][:, 2].mean().item(), rel=1e-5)


# ---- the plans -----------------------------------------------------------------------------------------------------------------------
def _plan_check(inf, run_segment, run_evaluate, hw, what):
    n = 3
    x, t = R.case("ring", (2, n, *hw))
    stack = t.to(DEV)                                            # (2, n, 1, H, W): head 1's targets above head 0's in memory
    before = run_segment()
    for order, (et, mt) in (("ascending", (stack[0], stack[1])), ("descending", (stack[1], stack[0]))):
        for tol in (0, 1):
            out = run_evaluate(et, mt, tol)
            torch.cuda.synchronize()
            assert set(out) == {"edges", "masks"}
            for name, tt in (("edges", et), ("masks", mt)):
                ref = R.reference(before[name].cpu(), tt.cpu(), tol=tol)
                assert out[name]["counts"].shape == (n, 6) and out[name]["counts"].dtype == torch.int32
                _against({k: v.cpu() for k, v in out[name].items()}, ref, f"{what} {name} {order} tol {tol}")
    after = run_segment()
    for k in before:
        assert torch.equal(before[k], after[k]) if before[k].dtype == torch.bool else same_bits(before[k], after[k]), k
    counts = out["edges"]["counts"].cpu()
    assert counts[:, 0].min() > 0 or counts[:, 1].min() > 0, "the case exercises nothing"


def _be_net16():
    """``networks_BE.ComposeNet`` with head width 16 on a 32-channel feature map, eval state seeded as tests/be_infer_ref.seeded_net does"""
    from vae_play_amd import networks_BE
    torch.manual_seed(3)
    net = networks_BE.ComposeNet(networks_BE.FeatureNet(None, 32, 16))
    g = NB.gen(503)
    with torch.no_grad():
        for name, m in net.named_modules():
            if hasattr(m, "num_batches_tracked"):
                p = {}
                NB._bn(p, "", m.weight.numel(), g)
                for k, v in p.items():
                    getattr(m, k).copy_(v)
        for name, q in net.named_parameters():
            if ".predictor." in name and name.endswith(".bias"):
                q.copy_(torch.randn(q.shape, generator=g) * 0.3)
    return net.eval()


def test_be_plan_evaluate():
    import vae_play_amd as V
    h, w = 3, 5
    net = _be_net16().to(DEV)
    inf = V.FusedBEInference(net, 2, h, w)
    assert inf.width == 16
    x = torch.randn((3, 32, h, w), generator=NB.gen(91)).to(DEV)
    _plan_check(inf, lambda: inf.segment(x), lambda et, mt, tol: inf.evaluate(x, et, mt, tolerance=tol), (4 * h, 4 * w), "be plan")
    # a captured plan replays ``predict`` as a graph; the evaluation launches stay eager and give the same bits
    _, t = R.case("ring", (2, 3, 12, 20))
    et, mt = t[0].to(DEV), t[1].to(DEV)
    eager = inf.evaluate(x, et, mt, tolerance=1)
    inf.capture()
    replayed = inf.evaluate(x, et, mt, tolerance=1)
    for name in ("edges", "masks"):
        assert _same_result({k: v.cpu() for k, v in eager[name].items()}, {k: v.cpu() for k, v in replayed[name].items()}), name
    with pytest.raises(ValueError):
        inf.evaluate(x, torch.zeros(2, 1, 12, 20, device=DEV), torch.zeros(3, 1, 12, 20, device=DEV))
    with pytest.raises(ValueError):
        inf.evaluate(x, torch.zeros(3, 1, 12, 20, device=DEV), torch.zeros(3, 1, 12, 20, device=DEV), tolerance=5)


@pytest.mark.parametrize("with_y", (False, True), ids=("image", "embed"))
def test_font_plan_evaluate(with_y):
    import vae_play_amd as V
    S = 16
    net, imgs, y, _ = NF.net_case(S)
    net = copy.deepcopy(net).to(DEV).eval()
    x = imgs[:3].to(DEV)
    yy = {k: v[:3].to(DEV) for k, v in y.items()} if with_y else None
    inf = V.FusedFontInference(net, 2)
    _plan_check(inf, lambda: inf.segment(x, yy), lambda et, mt, tol: inf.evaluate(x, et, mt, yy, tolerance=tol), (S, S),
                f"font plan {'embed' if with_y else 'image'}")
