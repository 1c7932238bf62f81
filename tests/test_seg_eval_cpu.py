"""Host-side checks of the segmentation evaluation (vae_play_amd/seg_eval.py): the float64 restatement the GPU tests
compare with is itself pinned -- to torch's BCE-with-logits, a direct dice score and the reference's loss (tests/golden/seg_eval.npz) --
the committed cases can tell each planted fault from the right answer, and ``summarize`` and the validation need no GPU."""
import inspect

import pytest
import torch
import torch.nn.functional as F

from tests import seg_eval_ref as R
from tests.util import load_golden, t as as_tensor

TOLS = (0, 1, 3)


def _golden_cases():
    g = load_golden("seg_eval")
    return [(as_tensor(g[f"c{k}/logits"]), as_tensor(g[f"c{k}/targets"]), float(g[f"c{k}/loss32"]), float(g[f"c{k}/loss64"]))
            for k in range(int(g["n"]))]


def _family_cases():
    return [(fam, shape, *R.case(fam, shape)) for fam in R.FAMILIES for shape in R.SHAPES]


def test_restatement_against_torch_float64():
    for fam, shape, x, t in _family_cases():
        ref = R.reference(x, t)
        n = shape[0] * shape[1]
        x64, t64 = x.double().reshape(n, -1), t.double().reshape(n, -1)
        bce = F.binary_cross_entropy_with_logits(x64, t64, reduction="none")
        p = torch.sigmoid(x64)
        dice = (2 * (p * t64).sum(1) + 1.0) / (p.sum(1) + t64.sum(1) + 1.0)
        assert torch.allclose(ref["sums"][:, 0], bce.sum(1), rtol=1e-12, atol=0), (fam, shape)
        assert torch.allclose(ref["terms"][:, 0], bce.mean(1), rtol=1e-12, atol=0), (fam, shape)
        assert torch.allclose(ref["terms"][:, 1], dice, rtol=1e-12, atol=0), (fam, shape)
        assert torch.allclose(ref["terms"][:, 2], 0.5 * bce.mean(1) + 1 - dice, rtol=1e-12, atol=0), (fam, shape)


def test_mean_of_per_image_loss_is_the_reference_loss():
    cases = _golden_cases()
    assert len(cases) >= 8
    for x, t, loss32, loss64 in cases:
        got = R.reference(x, t)["terms"][:, 2].mean().item()
        assert abs(got - loss64) <= 1e-12 * abs(loss64), (got, loss64)
        assert abs(loss32 - loss64) <= 1e-5 * abs(loss64)                 # the fp32 evaluation of the same expression


def test_golden_inputs_are_the_seeded_families():
    g = load_golden("seg_eval")
    for k in range(int(g["n"])):
        x = as_tensor(g[f"c{k}/logits"])
        fam = ("ring", "sparse")[int(g[f"c{k}/family"])]
        xr, tr = R.case(fam, (1,) + tuple(x.shape[:1]) + tuple(x.shape[2:]), int(g[f"c{k}/seed"]))
        assert torch.equal(tr[0], as_tensor(g[f"c{k}/targets"]))           # (bits; the logits go through randn and libm)
        assert torch.allclose(xr[0], x, rtol=1e-6, atol=1e-6)


def test_families_give_distinct_unsaturated_counts():
    """what makes an equality test of the counts worth something: the tolerant match is neither the plain overlap nor everything"""
    x, t = R.case("ring", (2, 3, 12, 20))
    c = R.reference(x, t, tol=1)["counts"]
    assert ((c[:, 3] > c[:, 2]) & (c[:, 3] < c[:, 0])).any() and ((c[:, 4] > c[:, 2]) & (c[:, 4] < c[:, 1])).any(), c
    x, t = R.case("sparse", (2, 3, 12, 20))
    c = R.reference(x, t, tol=3)["counts"]
    assert ((c[:, 3] > c[:, 2]) & (c[:, 3] < c[:, 0])).sum() >= 4 and len({tuple(r) for r in c.tolist()}) == c.shape[0], c


def test_tolerance_zero_is_the_plain_overlap():
    for fam, shape, x, t in _family_cases():
        c = R.reference(x, t, tol=0)["counts"]
        assert torch.equal(c[:, 3], c[:, 2]) and torch.equal(c[:, 4], c[:, 2])


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_changes_a_count(fault):
    """every fault a tiled, vectorised kernel can have changes a count on at least one committed case"""
    cases = [(x, t, tol) for _, _, x, t in _family_cases() for tol in TOLS] + list(R.explicit_cases().values())
    x, t = R.case("sparse", (1, 2, 5, 7))
    cases.append((torch.where(torch.rand(x.shape, generator=torch.Generator().manual_seed(3)) < 0.2, torch.tensor(0.5), x), t, 1))
    hit = sum(not torch.equal(R.reference(x, t, tol=tol)["counts"], R.reference(x, t, tol=tol, fault=fault)["counts"]) for x, t, tol in cases)
    assert hit >= 1, fault


def test_explicit_cases_isolate_their_fault():
    ex = R.explicit_cases()
    for name in ("wrap", "image_leak", "head_leak"):
        x, t, tol = ex[name]
        good, bad = R.reference(x, t, tol=tol)["counts"], R.reference(x, t, tol=tol, fault=name)["counts"]
        assert good[:, 3].sum() == 0 and good[:, 4].sum() == 0 and bad[:, 3].sum() == 1 and bad[:, 4].sum() == 1, name
    x, t, tol = ex["tail"]
    assert R.reference(x, t)["counts"][0].tolist() == [1, 1, 0, 0, 0, 0]
    assert R.reference(x, t, fault="drop_tail")["counts"][0, 0] == 0
    x, t, tol = ex["nan"]
    assert R.reference(x, t)["counts"][0].tolist() == [1, 2, 1, 1, 1, 1]
    assert R.reference(x, t, fault="nan_pred")["counts"][0, 0] == 2
    x, t, tol = ex["at_threshold"]
    assert R.reference(x, t)["counts"][0, 0] == 5 and R.reference(x, t, fault="gt")["counts"][0, 0] == 1


# ---- summarize -----------------------------------------------------------------------------------------------------------------------
def _result(counts, sums=None, terms=None):
    n = len(counts)
    return {"counts": torch.tensor(counts, dtype=torch.int32), "sums": torch.tensor(sums or [[0.0, 0.0, 0.0, 0.0]] * n),
            "terms": torch.tensor(terms or [[0.0, 1.0, 0.0]] * n)}


def test_summarize_on_hand_made_counts():
    from vae_play_amd import seg_eval
    #            |P| |T| both mp mt nonfinite
    s = seg_eval.summarize(_result([[4, 8, 2, 3, 4, 0], [6, 2, 2, 6, 1, 0]]))
    assert set(s) == set(seg_eval.FIGURES) and all(set(v) == {"micro", "macro"} and isinstance(v["micro"], float) for v in s.values())
    assert s["precision"] == {"micro": 4 / 10, "macro": (2 / 4 + 2 / 6) / 2}
    assert s["recall"] == {"micro": 4 / 10, "macro": (2 / 8 + 2 / 2) / 2}
    assert s["iou"] == {"micro": 4 / 16, "macro": (2 / 10 + 2 / 6) / 2}
    f = lambda a, b: 2 * a * b / (a + b)                                           # noqa: E731
    assert s["f1"]["micro"] == pytest.approx(0.4, rel=1e-15) and s["f1"]["macro"] == pytest.approx((f(0.5, 0.25) + f(1 / 3, 1.0)) / 2, rel=1e-15)
    assert s["boundary_precision"] == {"micro": 9 / 10, "macro": (3 / 4 + 1.0) / 2}
    assert s["boundary_recall"] == {"micro": 5 / 10, "macro": (4 / 8 + 1 / 2) / 2}
    assert s["boundary_f"]["micro"] == pytest.approx(f(0.9, 0.5), rel=1e-15)


def test_summarize_zero_denominators_and_harmonic_zero():
    from vae_play_amd import seg_eval
    s = seg_eval.summarize(_result([[0, 0, 0, 0, 0, 0]]))                           # nothing predicted, nothing to find: all right
    for k in ("iou", "precision", "recall", "f1", "boundary_precision", "boundary_recall", "boundary_f"):
        assert s[k] == {"micro": 1.0, "macro": 1.0}, k
    s = seg_eval.summarize(_result([[5, 3, 0, 0, 0, 0]]))                           # disjoint: precision 0, recall 0, harmonic mean 0
    assert s["precision"]["micro"] == 0.0 and s["recall"]["micro"] == 0.0 and s["f1"] == {"micro": 0.0, "macro": 0.0}
    assert s["boundary_f"] == {"micro": 0.0, "macro": 0.0}
    s = seg_eval.summarize(_result([[0, 3, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0]]))
    assert s["precision"] == {"micro": 0.0, "macro": 0.5} and s["recall"] == {"micro": 0.0, "macro": 0.5}


def test_summarize_loss_terms_micro_and_macro():
    from vae_play_amd import seg_eval
    x, t = R.case("ring", (1, 3, 12, 20))
    ref = R.reference(x, t, smooth=2.0)
    s = seg_eval.summarize(ref, smooth=2.0)
    for k, name in enumerate(seg_eval.TERMS):
        assert s[name]["macro"] == pytest.approx(ref["terms"][:, k].mean().item(), rel=1e-14)
    tot = ref["sums"].sum(0)
    dice = ((2 * tot[1] + 2.0) / (tot[2] + tot[3] + 2.0)).item()
    assert s["dice"]["micro"] == pytest.approx(dice, rel=1e-14)
    assert s["bce"]["micro"] == pytest.approx(tot[0].item() / (3 * 240), rel=1e-14)
    assert s["loss"]["micro"] == pytest.approx(0.5 * tot[0].item() / (3 * 240) + 1 - dice, rel=1e-13)
    with pytest.raises(ValueError):
        seg_eval.summarize({"sums": torch.zeros(2, 4), "terms": torch.zeros(2, 3), "counts": torch.zeros(3, 6)})


# ---- validation and signatures -------------------------------------------------------------------------------------------------------
def test_every_value_error():
    from vae_play_amd import seg_eval
    x, t = torch.zeros(2, 1, 4, 6), torch.zeros(2, 1, 4, 6)
    assert seg_eval.check_inputs(x, t) == (2, 4, 6)
    bad = [((x.double(), t), {}), ((x, t.half()), {}), ((x[:, 0], t), {}), ((x, t[:1]), {}), ((x, torch.zeros(2, 1, 6, 4)), {}),
           ((torch.zeros(2, 2, 4, 6), torch.zeros(2, 2, 4, 6)), {}), ((torch.zeros(0, 1, 4, 6), torch.zeros(0, 1, 4, 6)), {}),
           ((x.numpy(), t), {}), ((torch.zeros(2, 1, 4, 12)[..., ::2], t), {}), ((x, torch.zeros(2, 1, 6, 4).transpose(2, 3)), {}),
           ((x, torch.zeros(2, 1, 4, 6, device="meta")), {}),
           ((x, t), {"tolerance": 5}), ((x, t), {"tolerance": -1}), ((x, t), {"tolerance": 1.0}), ((x, t), {"tolerance": True}),
           ((x, t), {"threshold": float("nan")}), ((x, t), {"threshold": float("inf")}), ((x, t), {"target_threshold": float("-inf")})]
    for args, kw in bad:
        with pytest.raises(ValueError):
            seg_eval.segmentation_metrics(*args, **kw)
    big = torch.zeros(1).expand(1, 1, 4097, 4096)
    with pytest.raises(ValueError, match="2\\^24"):
        seg_eval.check_planes(big, "logits")


def test_cpu_tensors_are_refused_not_computed():
    from vae_play_amd import _lib, seg_eval
    with pytest.raises(_lib.VaePlayHipError):
        seg_eval.segmentation_metrics(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2))


def test_public_signatures():
    import vae_play_amd as V
    from vae_play_amd import seg_eval
    assert V.segmentation_metrics is seg_eval.segmentation_metrics and V.summarize is seg_eval.summarize
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]       # noqa: E731
    E = inspect.Parameter.empty
    assert sig(V.segmentation_metrics) == [("logits", E), ("targets", E), ("threshold", 0.5), ("tolerance", 0), ("bce_weight", 0.5),
                                           ("smooth", 1.0), ("target_threshold", 0.5)]
    assert sig(V.summarize)[0] == ("result", E) and all(d is not E for _, d in sig(V.summarize)[1:])
    tail = [("threshold", 0.5), ("tolerance", 0), ("bce_weight", 0.5), ("smooth", 1.0)]
    assert sig(V.FusedBEInference.evaluate) == [("self", E), ("x", E), ("edge_targets", E), ("mask_targets", E)] + tail
    assert sig(V.FusedFontInference.evaluate) == [("self", E), ("x", E), ("edge_targets", E), ("mask_targets", E), ("y", None)] + tail
