"""What mcx_fused_create decides for the books of fused_plan_cases.py, against the record in tests/golden/fused_describe.json
(written by tests/golden/gen_fused_describe_golden.py): per date straight-line or interpreted and the FastDate flag bits, the
prefetch pieces, the program slot, the cva-date table, the record count, and the kernel route of the four (inject, simulate)
pairs.  Exact comparison: the plan is integers.  No main pass runs."""
import json
import os
import re

import pytest

import fused_plan_cases as fpc
from mcx import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "fused_describe.json")) as _f:
    GOLDEN = json.load(_f)


def test_flag_names_match_the_header():
    """mcx/_abi.py FD_* = include/mcx.h MCX_FD_*, and the record was written for exactly the cases listed"""
    text = open(os.path.join(ROOT, "include", "mcx.h")).read()
    header = {name: int(val) for name, val in re.findall(r"\bMCX_(FD_[A-Z_]+) = (\d+)", text)}
    assert len(header) == 11 and sorted(header.values()) == [1 << k for k in range(11)], header
    assert {n: getattr(_abi, n) for n in header} == header
    assert set(GOLDEN) == set(fpc.CASES)
    for name in fpc.NEED_VPOLY:
        assert fpc.has_vpoly(GOLDEN[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(fpc.CASES))
def test_plan_matches_the_record(name, hip):
    got, want = fpc.describe(name, hip), GOLDEN[name]
    assert set(got) == set(want), (name, sorted(got), sorted(want))
    for key in sorted(want):
        assert got[key] == want[key], (name, key, got[key], want[key])
