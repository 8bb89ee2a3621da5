"""Host side of the product-batched forward-mode regression (mcx_tangent_lsm_batch; mcx/aad.py stateless_lsm_jobs and the
SimulationController.batch_tangent_lsm routes), without a GPU.  The CPU oracle has no dual kernels at all (no tangent_paths /
tangent_lsm / tangent_eval), so the batched route itself runs in tests/test_tangent_batch_gpu.py only; here: the job table against
a restatement of the per-job loop's arguments, the 72-product fixture and its mcx restatement against the reference's autograd
through the route the oracle takes (common-random-number bumps), the unchanged refusal of a backend without the batch entry, and
the ABI surface."""
import os
import re
import types

import numpy as np
import pytest

import cases
import large_cva_cases
from mcx import _abi, _native
from test_oracle_golden import check_lsm_sensitivities


def test_job_table_is_what_the_per_job_loop_passes_on_mixed_cva(oracle):
    from mcx.aad import stateless_lsm_jobs
    sc, _ = cases.make_controller("mixed_cva", oracle)
    sc.run_simulation()
    plan, storage_plan = sc._regression_plan()              # what run_with_tangent_book regresses on (no storage in this book)
    K = sc.book_plan.n_basis
    assert len(plan) == 4 and K == 3 and not storage_plan
    x_ids = sorted({x for _, _, _, atoms in plan for _, x in atoms})
    # ranges as lsm_stats would return them, the first atom degenerate (every path at one value, as at the calibration date)
    x_range = {x: ((0.25 * x - 1.0, 0.25 * x + 0.5 + 0.125 * k) if k else (1.5, 1.5)) for k, x in enumerate(x_ids)}
    table, keep = stateless_lsm_jobs(plan, x_range, sc._expo_coeff_base, K)
    assert table.dtype == _abi.TANGENT_LSM_JOB_DTYPE
    want, want_keep = [], []
    for p_i, p, sched, atoms in plan:                       # the loop of run_with_tangent_book, restated
        pdates = np.asarray([float(t) for t in p.product_timeline])
        for (t_reg, _r0, _r1, _prod_idx, expo_idx), (num, x) in zip(sched, atoms):
            if expo_idx is None:
                continue
            xmin, xmax = x_range[x]
            degenerate = not (xmax > xmin)
            shift = 0.5 * (xmin + xmax) if not degenerate else xmin
            scale = 2.0 / (xmax - xmin) if not degenerate else 1.0
            want.append((p_i, int(np.searchsorted(pdates, t_reg, side="right")), num, x, shift, scale))
            want_keep.append((sc._expo_coeff_base[p_i] + expo_idx * K, degenerate))
    assert len(want) >= 8 and any(d for _, d in want_keep) and not all(d for _, d in want_keep)
    assert [tuple(r) for r in table.tolist()] == want
    assert keep == want_keep
    # offsets: disjoint blocks of K coefficients inside the book's table
    offs = sorted(o for o, _ in keep)
    assert all(b - a >= K for a, b in zip(offs, offs[1:])) and offs[-1] + K <= len(sc.book_plan.coeffs)


def test_job_table_skips_products_with_states_and_dates_without_exposure_row():
    from mcx.aad import stateless_lsm_jobs
    prod = lambda states, dates: types.SimpleNamespace(get_num_states=lambda: states, product_timeline=dates)
    sched = [(0.0, 0, 0, None, 0), (0.5, 0, 1, None, None), (1.0, 1, 2, None, 1), (2.0, 2, 3, None, 2)]
    atoms = [(10, 20), (11, 21), (12, 22), (13, 23)]
    plan = [(0, prod(1, [0.5, 1.0, 2.0]), sched, atoms), (1, prod(3, [1.0]), sched, atoms), (2, prod(1, [1.0]), sched[:1], atoms[:1])]
    x_range = {20: (1.0, 1.0), 22: (-1.0, 3.0), 23: (0.0, 0.5)}
    table, keep = stateless_lsm_jobs(plan, x_range, {0: 100, 1: 200, 2: 300}, 2)
    assert [tuple(r) for r in table.tolist()] == [(0, 0, 10, 20, 1.0, 1.0), (0, 2, 12, 22, 1.0, 0.5), (0, 3, 13, 23, 0.25, 4.0),
                                                  (2, 0, 10, 20, 1.0, 1.0)]
    assert keep == [(100, True), (102, False), (104, False), (300, True)]
    empty, keep = stateless_lsm_jobs(plan[1:2], x_range, {1: 200}, 2)
    assert len(empty) == 0 and empty.dtype == _abi.TANGENT_LSM_JOB_DTYPE and keep == []


@pytest.fixture(scope="module")
def large_on_oracle(oracle):
    sc, g = large_cva_cases.make_controller(oracle)
    return sc, g, sc.run_simulation()


def test_large_cva_fixture_against_reference_autograd_on_the_oracle(large_on_oracle):
    """72 products, the reference's recorded draws: the oracle (no dual kernels: common-random-number bumps) meets the reference's
    autograd under the bounds of every LSM sensitivity fixture — tests/large_cva_cases.py restates the book faithfully and
    large_cva_aad.npz replays"""
    sc, g, res = large_on_oracle
    assert len(sc.products) == 72 and sc.timings.get("tangent") is False
    assert set(g.files) == {"z_pre", "z_main", "param_names", "result_0_0", "grad_0_0"}
    assert g["z_pre"].shape[1:] == (256, 3) and g["z_main"].shape[1:] == (256, 3)
    check_lsm_sensitivities(sc, g, res)


def test_fixture_is_no_larger_than_mixed_cva():
    size = lambda n: os.path.getsize(os.path.join(cases.GOLDEN, n + ".npz"))
    assert size("large_cva_aad") <= size("mixed_cva") and size("large_cva_aad") <= 1 << 20


@pytest.mark.parametrize("flag", [None, True])
def test_backend_without_batch_entry_refuses_the_large_book_as_before(oracle, flag):
    from mcx.aad import _NoTangentForm, run_with_tangent_book
    assert not hasattr(oracle, "tangent_lsm_batch")
    sc, _ = large_cva_cases.make_controller(oracle, inject=False)
    sc.batch_tangent_lsm = flag
    with pytest.raises(_NoTangentForm, match="products"):
        run_with_tangent_book(sc)


def test_route_choice():
    from mcx.aad import _NoTangentForm, _batch_tangent_lsm
    able, unable = types.SimpleNamespace(tangent_lsm_batch=None), types.SimpleNamespace()
    sc = lambda n, flag, be: types.SimpleNamespace(products=[0] * n, batch_tangent_lsm=flag, backend=be)
    assert [_batch_tangent_lsm(sc(n, None, able)) for n in (1, 64, 65, 180)] == [False, False, True, True]
    assert [_batch_tangent_lsm(sc(n, True, able)) for n in (1, 64, 65)] == [True, True, True]
    assert [_batch_tangent_lsm(sc(n, False, be)) for n in (1, 65) for be in (able, unable)] == [False] * 4
    assert _batch_tangent_lsm(sc(64, None, unable)) is False
    for n, flag in ((65, None), (3, True)):
        with pytest.raises(_NoTangentForm, match="products"):
            _batch_tangent_lsm(sc(n, flag, unable))


def test_controller_default_flag(oracle):
    sc, _ = cases.make_controller("mixed_cva", oracle)
    assert sc.batch_tangent_lsm is None


def test_abi_surface():
    assert "mcx_tangent_lsm_batch" in _native._EXPORTS
    header = open(os.path.join(os.path.dirname(cases.GOLDEN), os.pardir, "include", "mcx.h")).read()
    assert re.search(r"#define\s+MCX_ABI_VERSION\s+6\b", header) and _abi.ABI_VERSION == 6
    assert re.search(r"int\s+mcx_tangent_lsm_batch\(mcx_handle\*", header) and "MCX_TANGENT_BATCH_PARTIAL_BYTES" in header
    m = re.search(r"typedef struct \{([^}]*)\} mcx_tangent_lsm_job;", header)
    fields = [f.strip() for part in m.group(1).split(";") if part.strip() for f in part.strip().split(" ", 1)[1].split(",")]
    assert fields == list(_abi.TANGENT_LSM_JOB_DTYPE.names)
    assert hasattr(_native.HipBackend, "tangent_lsm_batch")
