"""Date-batched LSM under several (emulated) path-shard ranks: mcx_lsm_dates_moments -> ONE all-reduce -> mcx_lsm_solve_batch.

The off route of a book of four or more products under device collectives is mcx_lsm_step_batch_dev per step, which tiles each
rank's paths as mcx_lsm_dates_moments does, and the emulated all-reduce sums the ranks' tensors element by element in rank order:
the all-reduced moments of the two routes are the same bits, so the results are."""
import numpy as np
import pytest

import cases
from emulated_ranks import run_ranks
from mcx.maths.regression import PolyomialRegression

pytestmark = pytest.mark.gpu


def _results(res):
    return [[np.array(m, dtype=float) for m in ns] for ns in res.results]


def _on_ranks(world, build, flag):
    from mcx import _native

    def make(rank):
        sc = build(_native.HipBackend(0))
        sc.date_batched_lsm = flag
        return sc

    def body(sc, rank):
        res = sc.run_simulation()
        return _results(res), dict(sc.lsm_routes), [c.numpy().copy() for c in sc.regression_coeffs]

    return run_ranks(world, make, body)


def _assert_same(out_a, out_b):
    for (ra, _, ca), (rb, _, cb) in zip(out_a, out_b):
        for ns_a, ns_b in zip(ra, rb):
            for a, b in zip(ns_a, ns_b):
                assert np.array_equal(a, b, equal_nan=True), (a, b)
        for a, b in zip(ca, cb):
            assert np.array_equal(a, b)


def test_netting_on_three_ranks_is_bitwise_the_flag_off_run(hip):
    def build(be):
        sc, _ = cases.make_controller("netting", be, inject=False)
        sc.materialize = False
        sc.num_paths_mainsim, sc.num_paths_presim = 20002, 8001
        return sc

    single = build(hip)
    ref = _results(single.run_simulation())
    off, calls_off = _on_ranks(3, build, False)
    on, calls_on = _on_ranks(3, build, True)
    n_systems = sum(len(s) for _, _, s, _ in single._regression_plan()[0])
    for (_, routes_on, _), (_, routes_off, _) in zip(on, off):
        assert routes_on == {"dates": n_systems, "batched_steps": 0, "per_product": 0}
        assert routes_off["dates"] == 0 and routes_off["batched_steps"] > 0
    _assert_same(on, off)
    # one collective instead of one per step of the batched route
    assert calls_on["all_reduce"] == calls_off["all_reduce"] - (off[0][1]["batched_steps"] - 1)
    for got, _, _ in on:                                                  # against the one-shard run: tests/test_emulated_ranks.py's bounds
        for ns_r, ns_g in zip(ref, got):
            for m_r, m_g in zip(ns_r, ns_g):
                assert np.allclose(m_r[:, 0], m_g[:, 0], rtol=1e-9, atol=1e-12), (m_r[:, 0], m_g[:, 0])
                assert np.allclose(m_r[:, 1], m_g[:, 1], rtol=1e-6, atol=1e-11, equal_nan=True)


def test_irs_cva_on_three_ranks_regresses_in_one_collective(hip):
    def build(be):
        sc, _ = cases.make_controller("irs_cva", be, inject=False)
        sc.materialize = False
        sc.num_paths_mainsim, sc.num_paths_presim = 12001, 6001
        return sc

    probe = build(hip)
    probe.prepare()
    (_p_i, _p, sched, _atoms), = probe._regression_plan()[0]
    L = len(sched)
    assert L > 1
    off, calls_off = _on_ranks(3, build, False)
    on, calls_on = _on_ranks(3, build, True)
    assert all(r[1] == {"dates": L, "batched_steps": 0, "per_product": 0} for r in on)
    assert all(r[1] == {"dates": 0, "batched_steps": 0, "per_product": 1} for r in off)
    assert calls_on["all_reduce"] == calls_off["all_reduce"] - (L - 1), (calls_on, calls_off, L)
    assert calls_on["all_gather"] == calls_off["all_gather"]
    # the off route (mcx_lsm_step) tiles differently: the same terms in another order, under the one-shard bounds
    for (ra, _, _), (rb, _, _) in zip(on, off):
        for ns_a, ns_b in zip(ra, rb):
            for a, b in zip(ns_a, ns_b):
                assert np.allclose(a[:, 0], b[:, 0], rtol=1e-9, atol=1e-12) and np.allclose(a[:, 1], b[:, 1], rtol=1e-6, atol=1e-11, equal_nan=True)


def test_a_rank_without_pre_simulation_paths_takes_part(hip):
    """3 ranks, 2 pre-simulation paths (the third rank receives none), a degree-0 basis (K = 1: two paths determine the system).
    netting: the off route is the product-batched one, so the runs are bitwise equal"""
    def build(be):
        ns, model, rm = cases.netting()
        sc = cases.SimulationController(ns, model, rm, 3001, 2, 1, cases.A, backend=be, regression_function=PolyomialRegression(degree=0))
        return sc

    off, calls_off = _on_ranks(3, build, False)
    on, calls_on = _on_ranks(3, build, True)
    assert on[2][1]["dates"] > 0 and calls_on["all_reduce"] < calls_off["all_reduce"]
    assert all(np.isfinite(m).all() for r, _, _ in on for ns in r for m in ns)
    _assert_same(on, off)
