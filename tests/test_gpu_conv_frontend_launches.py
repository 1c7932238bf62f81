"""The autograd convolution front end launches what it launched before functional.py's four convolution Functions became two
(_Conv, _ConvT) over one dense core: per case of tools/record_conv_launches.py -- one layer per route of functional._conv_route /
_convt_route, forward and backward on 2 images of 8 x 8 -- the C-ABI calls, their scalar arguments and which of the case's tensors
each pointer is must equal tests/golden/conv_frontend_launches.json, recorded with the same tool on the revision before the
refactor (entry names canonicalised by the identities of the C side that the tool's docstring lists).

One deliberate edit to that log: conv2d's zero-padded route used to return its bias gradient as a fresh tensor even for a bias that
lives in an optim.FlatArena ("tmp" in the log: autograd copies it into ``.grad``); it now writes the arena slice ("db@arena") like
every other route."""
import copy
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_conv_launches", os.path.join(ROOT, "tools", "record_conv_launches.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)

with open(os.path.join(ROOT, "tests", "golden", "conv_frontend_launches.json")) as _f:
    GOLDEN = json.load(_f)

PADDED_ARENA = "conv2d-3x3-10to16-padded-in-arena-bf16x3"


def _expected(name):
    log = copy.deepcopy(GOLDEN[name])
    if name == PADDED_ARENA:
        entry, args = log[-1]
        assert entry == "vp_colsum_f32" and args[1] == "tmp", "the recorded bias gradient of the padded route: a fresh tensor"
        args[1] = "db@arena"
    return log


def test_golden_and_recorder_list_the_same_cases():
    assert sorted(GOLDEN) == sorted(REC.CASE_NAMES)


@pytest.mark.parametrize("case", REC.CASES, ids=REC.CASE_NAMES)
def test_front_end_launches_match_the_recorded_log(case):
    log, _ = REC.run_case(case)
    want = _expected(case["name"])
    assert len(log) == len(want), f"{len(log)} launches, recorded {len(want)}: {[l[0] for l in log]} vs {[l[0] for l in want]}"
    for i, (got, exp) in enumerate(zip(log, want)):
        assert got == exp, f"launch {i}: {got} != recorded {exp}"
