"""Page compositing on the GPU (csrc/be_page.hip, vae_play_amd.be_page.compose_page, FusedBEInference.segment_page): byte for byte
against the reference's own arrays (tests/golden/be_page_*.npz) and against the serial restatement (tests/be_page_ref.py, which
tests/test_be_page_cpu.py holds to those arrays).  Every comparison is torch.equal."""
import numpy as np
import pytest
import torch

from tests import be_infer_ref as N
from tests import be_page_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256


def _dev(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


def _run(case, threshold=0.5, out=None, meta_as="tensor"):
    import vae_play_amd as V
    conv = (lambda v: None if v is None else torch.from_numpy(v)) if meta_as == "tensor" else (lambda v: None if v is None else v.tolist())
    page = V.compose_page(_dev(case["edges"]), _dev(case.get("masks")), conv(case["recon_info"]), conv(case["boxes"]), conv(case["labels"]),
                          tuple(int(v) for v in case["page_hw"]), original_boxes=conv(case.get("original_boxes")),
                          page_masks=_dev(case.get("page_masks")), variant=case["variant"], threshold=threshold, out=out)
    torch.cuda.synchronize()
    return page


def _same(page, want, what):
    want = torch.from_numpy(want)
    assert page.dtype == torch.uint8 and tuple(page.shape) == tuple(want.shape)
    got = page.cpu()
    assert torch.equal(got, want), f"{what}: {int((got != want).any(dim=2).sum())} of {want.shape[0] * want.shape[1]} pixels differ"


class _Guarded:
    """an (H, W, 3) page between two runs of sentinel bytes, ``shift`` bytes past a 16-byte boundary"""

    def __init__(self, H, W, shift=0):
        n = H * W * 3
        self.buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.page = self.buf[GUARD + shift:GUARD + shift + n].view(H, W, 3)
        self.n, self.shift = n, shift
        assert self.page.data_ptr() % 16 == shift

    def check(self):
        lo, hi = self.buf[:GUARD + self.shift], self.buf[GUARD + self.shift + self.n:]
        assert bool((lo == 0xA5).all()) and bool((hi == 0xA5).all()), "the page was written out of bounds"


@pytest.mark.parametrize("kind", list(R.KINDS))
def test_golden_pages(kind):
    """the reference's own output, every page of the fixture"""
    variant, _ = R.KINDS[kind]
    for k, p in enumerate(R.golden_pages(kind)):
        case = dict(p, variant=variant)
        if kind == "edge":
            case["masks"] = None                        # (variant "edge" takes no content logits)
        _same(_run(case, meta_as="tensor" if k % 2 else "list"), p["page"], f"{kind} page {k}")


@pytest.mark.parametrize("H,W,S", R.PAGES)
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_standard_pages_vs_restatement(kind, H, W, S):
    """tests/be_page_ref.standard_case lists what its six bubbles cover; the page lies between sentinels, once on a 16-byte boundary
    (the white runs take 16-byte stores) and once 4 bytes past one"""
    case = R.standard_case(kind, H, W, S)
    want = R.expected(case)
    assert (want == 255).all(axis=2).any() and {0, 1, 3, 255} <= set(want[..., 1].ravel().tolist())
    assert np.isnan(case["edges"]).any() and (case["edges"] == 0.5).any()
    for shift in (0, 4):
        g = _Guarded(H, W, shift)
        page = _run(case, out=g.page)
        assert page is g.page                           # out= is the result
        g.check()
        _same(page, want, f"{kind} {H}x{W} S{S} shift {shift}")
    # another threshold moves the bits of the logit kinds and nothing else
    _same(_run(case, threshold=0.75), R.expected(case, threshold=0.75), f"{kind} {H}x{W} S{S} threshold 0.75")


@pytest.mark.parametrize("kind", list(R.KINDS))
def test_one_pixel_wide_page_and_empty_batch(kind):
    case = R.column_case(kind, 33)
    g = _Guarded(33, 1)
    _same(_run(case, out=g.page), R.expected(case), f"{kind} 33x1")
    g.check()
    # b == 0: a white page, whatever the buffer held
    variant, source = R.KINDS[kind]
    empty = dict(variant=variant, page_hw=(35, 47), edges=np.zeros((0, 1, 8, 8), dtype=np.float32), masks=np.zeros((0, 1, 8, 8), dtype=np.float32),
                 recon_info=np.zeros((0, 3), dtype=np.int64), boxes=np.zeros((0, 4), dtype=np.int64), labels=np.zeros((0,), dtype=np.int64))
    empty["original_boxes" if source == "original_boxes" else "page_masks"] = (
        np.zeros((0, 4), dtype=np.int64) if source == "original_boxes" else np.zeros((0, 35, 47), dtype=np.uint8))
    g = _Guarded(35, 47)
    g.page.fill_(7)
    page = _run(empty, out=g.page)
    g.check()
    assert bool((page == 255).all())


@pytest.mark.parametrize("kind", list(R.KINDS))
def test_three_hundred_bubbles(kind):
    """the descriptor table spans five LDS loads; the page is several workgroups"""
    case = R.random_case(kind, 96, 131, 20, 300)
    want = R.expected(case)
    assert 0.2 < (want != 255).any(axis=2).mean() < 0.8
    last = R.expected(case, rows=slice(0, 256))
    assert (last != want).any(), "the bubbles past the fourth table load change nothing: the case is too weak"
    _same(_run(case), want, f"{kind} b=300")


@pytest.mark.parametrize("kind", list(R.KINDS))
def test_chunks_onto_one_page_equal_one_call(kind):
    """white-init with the first bubbles, then continue with the rest == everything at once (a claimed pixel is never white)"""
    from ctypes import c_void_p
    from vae_play_amd import be_page
    H, W, S = R.PAGES[1]
    case = R.standard_case(kind, H, W, S)
    b = len(case["labels"])
    whole = _run(case)
    _same(whole, R.expected(case), "one call")
    table = be_page.page_descriptors(case["recon_info"], case["boxes"], case["labels"], (H, W), (S, S), case["original_boxes"],
                                     case["page_masks"] is not None, case["variant"]).to(DEV)
    e, m, pm = _dev(case["edges"]), _dev(case["masks"]), _dev(case["page_masks"])
    g = _Guarded(H, W)
    g.page.fill_(3)
    for i0, i1 in ((0, 1), (1, 4), (4, b)):
        be_page.launch(c_void_p(e[i0].data_ptr()), S * S, c_void_p(m[i0].data_ptr()), S * S, table[i0:], i1 - i0, None if pm is None else pm[i0:],
                       g.page, (S, S), 0.5, i0 == 0)
        torch.cuda.synchronize()
        _same(g.page, R.expected(case, rows=slice(0, i1)), f"{kind} after bubble {i1}")
    g.check()
    assert torch.equal(g.page, whole)


# ---- FusedBEInference.segment_page ------------------------------------------------------------------------------------------------
def _net_case(kind, n, h, w, seed=5):
    """n bubbles for crops whose logit planes are (4h, 4w): sizes around the planes' sides"""
    rng = np.random.default_rng(seed)
    H, W = 57, 75
    rows = []
    for i in range(n):
        bw, bh = int(rng.integers(8, 40)), int(rng.integers(8, 40))
        xmin, ymin = int(rng.integers(0, W - bw + 1)), int(rng.integers(0, H - bh + 1))
        size = max(bw, bh) + int(rng.integers(0, 3))
        ax, ay = int(rng.integers(0, size - bw + 1)), int(rng.integers(0, size - bh + 1))
        rows.append(((ax, ay, size), (xmin, ymin, xmin + bw, ymin + bh), 3 if i == 1 else 1 + i % 2, (xmin + 2, ymin + 3, xmin + bw - 1, ymin + bh - 2)))
    return R._case(rng, kind, H, W, 4 * h, 4 * w, rows)


@pytest.mark.parametrize("kind", list(R.KINDS))
def test_segment_page(kind):
    """n = batch_size + 3 crops through the plan, eager and captured: the page equals compose_page on the object's own segment(x)
    logits and the restatement on them; segment(x) is unchanged by it"""
    import vae_play_amd as V
    h, w = N.SHAPES[3]
    B = 2
    n = B + 3
    net = N.seeded_net("be").to(DEV)
    x = torch.randn((n, 256, h, w), generator=N.gen(91)).to(DEV)
    inf = V.FusedBEInference(net, B, h, w)
    before = inf.segment(x)
    # the logits of a seeded net are what they are: put the threshold where it splits them
    thr = float(torch.cat([before["edges"].flatten(), before["masks"].flatten()]).median())
    case = _net_case(kind, n, h, w)
    case["edges"], case["masks"] = before["edges"].cpu().numpy(), before["masks"].cpu().numpy()
    want = R.expected(case, threshold=thr)
    assert 0.05 < (want[..., 0] == 255).mean() < 0.999 and (want[..., 2] == 255).any() and (want[..., 0] == 0).any()
    meta = dict(original_boxes=None if case["original_boxes"] is None else torch.from_numpy(case["original_boxes"]),
                page_masks=_dev(case["page_masks"]), variant=case["variant"], threshold=thr)
    args = (torch.from_numpy(case["recon_info"]), torch.from_numpy(case["boxes"]), torch.from_numpy(case["labels"]), case["page_hw"])
    direct = V.compose_page(before["edges"], before["masks"], *args, **meta)
    _same(direct, want, "compose_page on segment(x)")
    for mode in ("eager", "captured"):
        if mode == "captured":
            inf.capture()
        g = _Guarded(*case["page_hw"])
        page = inf.segment_page(x, *args, out=g.page, **meta)
        torch.cuda.synchronize()
        g.check()
        _same(page, want, f"segment_page {mode}")
        assert torch.equal(page, direct)
        _same(inf.segment_page(x.contiguous(memory_format=torch.channels_last), *args, **meta), want, f"segment_page {mode} channels_last")
        after = inf.segment(x)
        assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before), f"segment(x) changed ({mode})"
    # no crops: a white page
    none = inf.segment_page(x[:0], [], [], [], case["page_hw"], original_boxes=[] if kind == "annot" else None,
                            page_masks=None if kind == "annot" else torch.zeros((0, *case["page_hw"]), dtype=torch.uint8, device=DEV),
                            variant=case["variant"])
    assert tuple(none.shape) == (*case["page_hw"], 3) and bool((none == 255).all())
    with pytest.raises(ValueError, match="bubbles"):
        inf.segment_page(x[:2], *args, **meta)
