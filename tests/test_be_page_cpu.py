"""Page compositing without a GPU: the serial restatement (tests/be_page_ref.py) against the arrays the reference's own paste
functions produced (tests/golden/be_page_*.npz, tools/gen_golden_be_page.py), the host-side validation of
``vae_play_amd.be_page.page_descriptors``, and the public signatures."""
import inspect
import sys

import numpy as np
import pytest
import torch

from tests import be_page_ref as R


def _descriptors(page, kind, **over):
    from vae_play_amd import be_page
    variant, _ = R.KINDS[kind]
    a = dict(recon_info=page["recon_info"], boxes=page["boxes"], labels=page["labels"], page_hw=tuple(int(v) for v in page["page_hw"]),
             logit_hw=page["edges"].shape[2:], original_boxes=page.get("original_boxes"), has_page_masks=page.get("page_masks") is not None,
             variant=variant)
    a.update(over)
    return be_page.page_descriptors(**a)


@pytest.mark.parametrize("kind", list(R.KINDS))
def test_restatement_equals_the_reference_arrays(kind):
    variant, _ = R.KINDS[kind]
    pages = R.golden_pages(kind)
    assert len(pages) >= 6
    seen = set()
    for k, p in enumerate(pages):
        hw = tuple(int(v) for v in p["page_hw"])
        assert max(hw) <= 96 and len(p["labels"]) <= 6 and p["edges"].shape[-1] in (8, 16, 20)
        out = R.compose(p["edges"], p.get("masks"), p["recon_info"], p["boxes"], p["labels"], hw, p.get("original_boxes"),
                        p.get("page_masks"), variant)
        assert out.dtype == np.uint8 and out.shape == p["page"].shape == (*hw, 3)
        assert np.array_equal(out, p["page"]), f"{kind} page {k}: {(out != p['page']).any(axis=2).sum()} pixels differ"
        seen |= set(int(v) for v in p["labels"])
        assert np.isnan(p["edges"]).any() and (p["edges"] == 0.5).any() or hw == (8, 8)
    assert 3 in seen and len(seen) >= 4


def test_the_generators_stubs_are_not_needed():
    """the restatement and the fixtures need numpy alone; neither cv2 nor torchvision is imported by anything here"""
    R.golden_pages("annot")
    import vae_play_amd.be_page  # noqa: F401
    assert "cv2" not in sys.modules and "test_BE_manga" not in sys.modules
    tv = sys.modules.get("torchvision")
    assert tv is None or getattr(tv, "__file__", None), "a stub torchvision is installed"
    names = {v.__name__ for v in vars(R).values() if inspect.ismodule(v)}
    assert names == {"numpy"}


@pytest.mark.parametrize("kind", list(R.KINDS))
def test_validation_accepts_the_fixtures_and_builds_the_table(kind):
    from vae_play_amd import be_page
    for p in R.golden_pages(kind):
        S = p["edges"].shape[-1]
        for as_tensor in (False, True):                # lists / arrays, and the CPU LongTensors the reference's loaders return
            q = {k: (torch.from_numpy(v) if as_tensor and v.dtype == np.int64 else v) for k, v in p.items()}
            if not as_tensor:
                q.update(recon_info=p["recon_info"].tolist(), boxes=p["boxes"].tolist(), labels=p["labels"].tolist())
            t = _descriptors(q, kind)
            assert t.dtype == torch.int32 and tuple(t.shape) == (len(p["labels"]), be_page.DESC_INTS) and not t.is_cuda
            t = t.numpy()
            assert np.array_equal(t[:, [0, 1]], p["recon_info"][:, :2]) and np.array_equal(t[:, 4:8], p["boxes"])
            assert np.array_equal(t[:, 12], p["labels"]) and not t[:, 14:].any()
            scale = t[:, 2:4].copy().view(np.float32)
            want = np.float32(S) / p["recon_info"][:, 2].astype(np.float32)
            assert np.array_equal(scale[:, 0], want) and np.array_equal(scale[:, 1], want)
            three = p["labels"] == 3
            want_kind = {"annot": (be_page.KIND_LOGITS, be_page.KIND_RECT), "mask": (be_page.KIND_LOGITS, be_page.KIND_PAGE_MASK),
                         "edge": (be_page.KIND_EDGE_LOGITS, be_page.KIND_PAGE_MASK)}[kind]
            assert np.array_equal(t[:, 13], np.where(three, want_kind[1], want_kind[0]))
            if kind == "annot":
                shift = p["recon_info"][:, :2] - p["boxes"][:, :2]
                rect = p["original_boxes"] + np.concatenate([shift, shift], axis=1)
                assert np.array_equal(t[three, 8:12], rect[three])


def _one(info=(1, 2, 12), box=(3, 4, 13, 12), label=1, obox=(4, 5, 9, 9), hw=(20, 30), kind="annot"):
    p = dict(recon_info=[list(info)], boxes=[list(box)], labels=[label], page_hw=hw, edges=np.zeros((1, 1, 8, 8), dtype=np.float32))
    if kind == "annot":
        p["original_boxes"] = [list(obox)]
    else:
        p["page_masks"] = np.zeros((1, *hw), dtype=np.uint8)
    return p, kind


BAD = {
    "box right of the page": _one(box=(21, 4, 31, 12)),
    "box below the page": _one(box=(3, 13, 13, 21)),
    "box with a negative corner": _one(box=(-1, 4, 9, 12)),
    "box of width 0": _one(box=(3, 4, 3, 12)),
    "box reversed in y": _one(box=(3, 12, 13, 4)),
    "anchor_x + width > size": _one(info=(3, 2, 12)),
    "anchor_y + height > size": _one(info=(1, 5, 12)),
    "negative anchor": _one(info=(-1, 2, 12)),
    "size 0": _one(info=(0, 0, 0)),
    "rectangle left of the crop square": _one(label=3, obox=(1, 5, 9, 9)),
    "rectangle beyond the crop square": _one(label=3, obox=(4, 5, 15, 9)),
    "rectangle beyond the crop square in y": _one(label=3, obox=(4, 5, 9, 15)),
    "rectangle reversed in x": _one(label=3, obox=(9, 5, 4, 9)),
    "rectangle reversed in y": _one(label=3, obox=(4, 9, 9, 5)),
    "label 256": _one(label=256),
    "label -1": _one(label=-1),
    "label 3 from a page mask, box 1 wide": _one(info=(1, 2, 12), box=(3, 4, 4, 12), label=3, kind="mask"),
    "label 3 from a page mask, box 1 high": _one(info=(1, 2, 12), box=(3, 4, 13, 5), label=3, kind="edge"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_validation_raises(name):
    page, kind = BAD[name]
    with pytest.raises(ValueError):
        _descriptors(page, kind)


def test_validation_of_sources_shapes_and_logits():
    from vae_play_amd import be_page
    good, kind = _one()
    assert _descriptors(good, kind).shape == (1, 16)
    # a label-3 rectangle that is empty, or touches the crop square's border, is fine; so is a 1 x 1 box away from the page-mask kinds
    _descriptors(_one(label=3, obox=(4, 5, 4, 9))[0], "annot")
    _descriptors(_one(label=3, obox=(2, 2, 14, 14))[0], "annot")
    _descriptors(_one(info=(0, 0, 1), box=(3, 4, 4, 5), label=1, kind="edge")[0], "edge")
    # size == 1 under label 3 with an original box: the reference computes it (the generator's probe; the last page of
    # be_page_annot.npz pins its bytes), so it is accepted
    _descriptors(_one(info=(0, 0, 1), box=(3, 4, 4, 5), label=3, obox=(3, 4, 4, 5))[0], "annot")
    # the wrong mask source for the variant
    for over in (dict(variant="result", original_boxes=None, has_page_masks=False), dict(variant="result", has_page_masks=True),
                 dict(variant="edge"), dict(variant="edge", original_boxes=None, has_page_masks=False),
                 dict(variant="edge", has_page_masks=True), dict(variant="overlay")):
        with pytest.raises(ValueError):
            _descriptors(good, kind, **over)
    # rows that do not line up, fractional metadata
    for over in (dict(labels=[1, 2]), dict(boxes=[[3, 4, 13]]), dict(original_boxes=[[4, 5, 9, 9]] * 2), dict(recon_info=[[1.0, 2.0, 12.0]]),
                 dict(page_hw=(0, 30)), dict(logit_hw=(0, 8))):
        with pytest.raises(ValueError):
            _descriptors(good, kind, **over)
    # logits: fp32 and contiguous, (b, 1, SH, SW)
    assert be_page.check_logits(torch.zeros((2, 1, 8, 8)), "edges", 2) == (8, 8)
    for bad in (torch.zeros((2, 1, 8, 8), dtype=torch.float64), torch.zeros((2, 1, 8, 8), dtype=torch.float16),
                torch.zeros((2, 1, 8, 16))[..., ::2], torch.zeros((2, 2, 8, 8)), torch.zeros((3, 1, 8, 8)), None):
        with pytest.raises(ValueError):
            be_page.check_logits(bad, "edges", 2)
    with pytest.raises(ValueError):
        be_page.check_page_masks(torch.zeros((1, 20, 30)), 1, (20, 30))
    with pytest.raises(ValueError):
        be_page.check_page_masks(torch.zeros((1, 20, 31), dtype=torch.uint8), 1, (20, 30))


def test_compose_page_refuses_on_the_host_before_it_needs_a_device():
    """the ValueErrors come first, and CPU logits are refused rather than composed anywhere else"""
    import vae_play_amd as V
    from vae_play_amd import _lib
    good, _ = _one()
    args = (good["recon_info"], good["boxes"], good["labels"], good["page_hw"])
    e = torch.zeros((1, 1, 8, 8))
    with pytest.raises(ValueError, match="contiguous"):
        V.compose_page(torch.zeros((1, 1, 8, 16))[..., ::2], e, *args, original_boxes=good["original_boxes"])
    with pytest.raises(ValueError, match="fp32"):
        V.compose_page(e.double(), e, *args, original_boxes=good["original_boxes"])
    with pytest.raises(ValueError, match="masks"):
        V.compose_page(e, None, *args, original_boxes=good["original_boxes"])
    with pytest.raises(ValueError, match="exactly one"):
        V.compose_page(e, e, *args)
    with pytest.raises(ValueError, match="leaves"):
        V.compose_page(e, e, good["recon_info"], [[25, 4, 35, 12]], good["labels"], good["page_hw"], original_boxes=good["original_boxes"])
    with pytest.raises(_lib.VaePlayHipError, match="HIP device"):
        V.compose_page(e, e, *args, original_boxes=good["original_boxes"])


def test_public_signatures():
    import vae_play_amd as V
    sig = inspect.signature(V.compose_page)
    assert list(sig.parameters) == ["edges", "masks", "recon_info", "boxes", "labels", "page_hw", "original_boxes", "page_masks", "variant",
                                    "threshold", "out"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(original_boxes=None, page_masks=None, variant="result", threshold=0.5, out=None)
    sig = inspect.signature(V.FusedBEInference.segment_page)
    assert list(sig.parameters)[:6] == ["self", "x", "recon_info", "boxes", "labels", "page_hw"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(original_boxes=None, page_masks=None, variant="result", threshold=0.5, out=None)
    assert "compose_page" in V.__all__
