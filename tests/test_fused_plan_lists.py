"""The launch lists of the three fused plans (FusedVAEStep, FusedVAEGANStep, FusedVAEInference), checked without a GPU against
tests/golden/fused_plans.json.gz -- recorded by tools/gen_golden_fused_plans.py from the PARENT of the change that shares the plans'
sections (vae_play_amd/sections.py): per case the same launches in the same order with the same arguments, tags, FLOP counts, side
slots, side arguments, hooks and waits, the same bytes of buffers, and every pointer of every launch inside memory the step owns
(``_bufs``), the model, a gradient arena, the shadow arena or the saturation flag.  The last is checked after a garbage collection:
a launch list holds raw addresses, so a tensor that a section builder allocated without registering it is freed memory by then."""
import gc
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import gen_golden_fused_plans as G  # noqa: E402  (the cases and the canonical form)

GOLDEN = json.loads(G.read_golden())


def test_fixture_holds_exactly_the_cases():
    assert list(GOLDEN) == G.CASE_NAMES
    assert all(rec["unresolved"] == 0 for rec in GOLDEN.values())


@pytest.mark.parametrize("case", G.CASES, ids=G.CASE_NAMES)
def test_plan_equals_parent_recording(case):
    want = GOLDEN[case["name"]]
    got = json.loads(json.dumps(G.record_case(case, collect=gc.collect)))
    assert got["unresolved"] == 0, [c[:2] + c[4:5] for c in got["calls"] if '"?"' in json.dumps(c)]
    assert got["env"] == want["env"] and got["attrs"] == want["attrs"]
    assert [c[:2] + c[4:5] for c in got["calls"]] == [c[:2] + c[4:5] for c in want["calls"]]      # (the readable diff first)
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {i}"
    assert got["bufs_bytes"] == want["bufs_bytes"]
    assert got["kept"] == want["kept"]
