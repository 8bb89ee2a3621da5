"""The draws and the step count of the cva-date kernel (kf_lean.hip: integer-built second uniform, scalar second Philox round
on the launch's one high path word, one rare-draw test per lane, no sub-steps after the last date that adds to the CVA) against
kf_lean's general kernel, which keeps the shared sub-step helpers and the full step table.  A pass without an output buffer takes
the cva-date route, the same pass with an output buffer the general one: the record arrays must agree bit for bit.  Only a launch
whose grid is the kernel's whole residency (4 blocks per CU) runs the new draws; a thinner one runs the cva-date kernel with the
staged draws of mcx_device.h and shares the trimmed step count and the launch rule.

The output buffer is the paths tensor.  A cashflow buffer also selects the general kernel, but it makes every date a cashflow
consumer, and lean_date (kf_common.h) then leaves the merged CVA increment relu(p) (S / N) (1 - Sc) for relu(p / N) S (1 - Sc):
another rounding, not another route.  Before the draws of the cva-date kernel were touched the two already differed in the last
bits of the second moment with a cashflow buffer (70001 paths from offset 0: s2 = 0x1.6d0f5fc95da82p-10 against
0x1.6d0f5fc95da80p-10; 4097 paths: 0x1.639c865518b80p-14 against 0x1.639c865518b7fp-14), with n, the shift and s1 equal.  With
the paths tensor the general kernel stores the states and keeps the merged increment."""
import numpy as np
import pytest

import cases
from mcx import _abi
from test_cva_date_kernel import _check, _irs_book

pytestmark = pytest.mark.gpu

LIVE = _abi.FD_MERGED | _abi.FD_EXERCISE | _abi.FD_STATE_EXPO      # FastDate flags: == FD_MERGED is the merged CVA increment (mcx_fused_create)


def _controller(be, timeline_end, n_main):
    """3-year quarterly payer swap, 2 sub-steps per interval; exposure dates up to timeline_end"""
    ns, model, rm = _irs_book(3.0, True, 0.25, 1.0)
    if timeline_end != 3.0:
        rm = cases.RiskMetrics([cases.CVAMetric("cp", 0.4)], exposure_timeline=np.arange(0.0, timeline_end + 1e-9, 0.25))
    sc = cases.SimulationController(ns, model, rm, n_main, 4096, 2, cases.E, backend=be)
    return sc


def _run_fused(hip, timeline_end, n_main):
    sc = _controller(hip, timeline_end, n_main)
    sc.main_plan = "fused"
    res = sc.run_simulation().results
    d = hip.fused_describe(sc._fused, False, True)
    assert d["kernel"] == "lean" and d["cva_dates"] and (d["valid"] == 1).all(), d
    return sc, res, d


@pytest.fixture(scope="module")
def book(hip):
    """the controller whose fused object and regression coefficients every path-count case below runs on"""
    return _run_fused(hip, 3.0, 4096)[0]


def _both_routes(hip, sc, path_offset, n):
    seed = sc._main_engine.seed
    plain = hip.fused_run(sc._fused, seed, path_offset, n)                      # the cva-date kernel
    paths = hip.empty(sc.sim_plan.n_dates, sc.sim_plan.n_state, n)
    general = hip.fused_run(sc._fused, seed, path_offset, n, paths=paths)       # kf_lean's general kernel
    assert plain.dtype == general.dtype and plain.shape == general.shape and len(plain) >= 1
    for name in plain.dtype.names:
        assert np.array_equal(plain[name], general[name]), (name, path_offset, n, plain[name], general[name])
    assert np.array_equal(plain, general)
    return plain


def _full_counts(hip):
    """path counts whose grid is the whole residency of the two-paths-per-lane kernel, 4 blocks per CU of 512-path tiles: one
    tile per block, and two tiles per block with a partial last tile.  Only such a launch runs the new draws (cva_draw_pairs);
    any other count is dealt to fewer blocks (launch_lean_shape) and runs the cva-date kernel with the staged draws"""
    full = 4 * hip.device_info()["n_cu"] * 512
    return [full, 2 * full - 255]


# one path per lane: dead lanes, one partial tile, many tiles; two paths per lane from 2 x CUs tiles of 512 paths on.  All of these
# are thin launches: the trimmed step count, the launch rule and the staged draws
@pytest.mark.parametrize("n", [1, 255, 257, 70001, 262144 + 1, 300001])
def test_path_counts_match_the_general_kernel(n, hip, book):
    _both_routes(hip, book, 0, n)


def test_full_grids_match_the_general_kernel(hip, book):
    """the new draws: integer-built uniform, scalar second Philox round, one rare-draw test"""
    for n in _full_counts(hip):
        _both_routes(hip, book, 0, n)


def test_non_zero_high_path_word(hip, book):
    """every lane's path index has high word 1: on a full grid the scalar second Philox round runs on a non-zero word"""
    for n in [70001] + _full_counts(hip)[:1]:
        a = _both_routes(hip, book, 2**32 + 12345, n)
        b = _both_routes(hip, book, 12345, n)
        assert not np.array_equal(a, b)      # (the high word reaches the draws)


def test_launch_that_straddles_a_high_word_runs_the_general_kernel(hip, book):
    """paths from 2^32 - 1000 on: no single high word, the pass falls back to the general kernel (thin and full grid)"""
    for n in [70001] + _full_counts(hip)[:1]:
        _both_routes(hip, book, 2**32 - 1000, n)


@pytest.mark.parametrize("timeline_end", [3.0, 2.0], ids=["timeline-to-maturity", "timeline-a-year-short"])
def test_step_count_follows_the_last_cva_date(timeline_end, hip, oracle):
    """Both books trim.  The CVA metric adds nothing at the last date of its timeline, so with exposure dates up to the maturity
    the cva-date kernel stops after the sub-steps of t = 2.75; with a timeline that stops a year earlier, after those of t = 1.75.
    Both equal the general kernel on the full step table, and both are what the oracle computes.  (No CVA book has an increment
    at its last simulated date, so the untrimmed count is reached only through the general kernel.)"""
    n = 70001
    sc, res, d = _run_fused(hip, timeline_end, n)
    live = (d["flags"] & LIVE) == _abi.FD_MERGED
    n_dead = 1 if timeline_end == 3.0 else 5
    assert live[:-n_dead].all() and not live[-n_dead:].any(), d          # 13 quarterly dates, the last n_dead without increment
    eng = sc._main_engine
    _both_routes(hip, sc, eng.path_offset, n)
    so = _controller(oracle, timeline_end, n)
    _check({"hip": res, "oracle": so.run_simulation().results}, ("trim", timeline_end))
