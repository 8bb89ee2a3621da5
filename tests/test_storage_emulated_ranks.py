"""A storage with its pre-simulation and main paths on three emulated ranks of uneven size (tests/emulated_ranks.py): the
several-ranks branch of the storage regression — per date mcx_storage_lsm_step -> all-reduce of the moments -> host solve ->
coefficient upload — must reproduce the single-shard run (one mcx_storage_lsm_run call), as test_emulated_ranks.py asserts for
exercise products."""
import numpy as np
import pytest

import storage_cases
from emulated_ranks import run_ranks


def _results(res):
    return [[np.array(m, dtype=float) for m in ns] for ns in res.results]


@pytest.mark.gpu
def test_storage_shift_on_three_emulated_ranks_matches_the_single_shard_run(hip):
    from mcx import _native

    def build(be):
        sc, _ = storage_cases.make_controller("storage_shift", be, inject=False)
        sc.materialize = False
        return sc

    single = build(hip)
    ref = _results(single.run_simulation())
    ref_coeffs = single.products[0].regression_coeffs.numpy().copy()

    def body(sc, rank):
        return _results(sc.run_simulation()), sc.products[0].regression_coeffs.numpy().copy()

    out, calls = run_ranks(3, lambda rank: build(_native.HipBackend(0)), body)
    assert calls["all_reduce"] >= len(ref_coeffs)              # the moments of every regression date crossed the ranks
    for rank, (got, coeffs) in enumerate(out):
        assert np.allclose(coeffs, ref_coeffs, rtol=1e-8, atol=1e-11 * np.abs(ref_coeffs).max()), (rank, np.abs(coeffs - ref_coeffs).max())
        for ns_r, ns_g in zip(ref, got):
            for m_r, m_g in zip(ns_r, ns_g):
                assert np.allclose(m_r[:, 0], m_g[:, 0], rtol=1e-9, atol=1e-12), (rank, m_r[:, 0], m_g[:, 0])
    for got, _ in out[1:]:
        for ns_a, ns_b in zip(out[0][0], got):
            for a, b in zip(ns_a, ns_b):
                assert np.array_equal(a, b, equal_nan=True)
