"""Host side of the date-batched LSM route (no GPU): the chain builder lsm_date_chains against the step-major tables of the
product-batched route, and the names / defaults the route adds."""
import os

import numpy as np

import cases
from mcx import _abi, _native, aad
from mcx.controller import controller as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N_LOCAL = 3, 40


class _Product:
    def __init__(self, S):
        self.S = S

    def get_num_states(self):
        return self.S


def _book():
    """six hand-made regression jobs: two stateless products of one class (shared schedule and atoms), an empty schedule, a
    schedule of one date, and exercise products of two and three states in between.  Atom 7's range is a point (degenerate)"""
    sched_a = [(2.0, 5, 5, None, 4), (1.0, 3, 5, 1, 2), (0.0, 0, 3, 0, 0)]
    atoms_a = [(10, 11), (8, 9), (6, 7)]
    sched_b = [(1.5, 2, 4, 1, None), (0.5, 0, 2, 0, 1)]
    atoms_b = [(12, 13), (14, 15)]
    sched_c = [(1.0, 0, 2, None, 2)]
    atoms_c = [(8, 9)]
    jobs = [(0, _Product(1), sched_a, atoms_a), (1, _Product(2), sched_b, atoms_b), (2, _Product(1), sched_a, atoms_a),
            (3, _Product(1), [], []), (4, _Product(1), sched_c, atoms_c), (5, _Product(3), sched_b, atoms_b)]
    x_range = {11: (-1.0, 3.0), 9: (0.5, 0.75), 7: (0.25, 0.25), 13: (1.0, 2.0), 15: (-2.0, 2.0)}
    reg_base = np.array([0, 100, 200, 300, 400, 500])
    expo_base = np.array([1000, 1100, 1200, 1300, 1400, 1500])
    return jobs, x_range, reg_base, expo_base


def test_chain_builder_orders_chain_major_and_keeps_the_remainder():
    jobs, x_range, reg_base, expo_base = _book()
    stateless, rest, jt, sj, chain_begin, w_len = C.lsm_date_chains(jobs, x_range, reg_base, expo_base, N_LOCAL, K)
    assert [j[0] for j in stateless] == [0, 2, 3, 4] and all(a is b for a, b in zip(stateless, [jobs[0], jobs[2], jobs[3], jobs[4]]))
    assert len(rest) == 2 and rest[0] is jobs[1] and rest[1] is jobs[5]                # the input minus the stateless jobs, in order
    assert chain_begin.dtype == np.int32 and chain_begin.tolist() == [0, 3, 6, 6, 7]   # (the empty schedule: an empty chain)
    assert jt.dtype == _abi.LSM_JOB_DTYPE and sj.dtype == _abi.LSM_SOLVE_JOB_DTYPE and len(jt) == len(sj) == 7
    assert w_len == 4 * N_LOCAL
    assert jt["product"].tolist() == [0, 0, 0, 2, 2, 2, 4]
    assert jt["w_offset"].tolist() == [0, 0, 0, N_LOCAL, N_LOCAL, N_LOCAL, 3 * N_LOCAL]  # one private row per chain
    # schedule order inside every chain
    assert jt["roll_begin"].tolist() == [5, 3, 0, 5, 3, 0, 0] and jt["roll_end"].tolist() == [5, 5, 3, 5, 5, 3, 2]
    assert jt["num_atom"].tolist() == [10, 8, 6, 10, 8, 6, 8] and jt["x_atom"].tolist() == [11, 9, 7, 11, 9, 7, 9]
    # centring: the midpoint and 2 / width, or (x0, 1) for the degenerate date
    assert jt["shift"][:3].tolist() == [1.0, 0.625, 0.25] and jt["scale"][:3].tolist() == [0.5, 8.0, 1.0]
    assert sj["degenerate"].tolist() == [0, 0, 1, 0, 0, 1, 0] and sj["x0"][2] == 0.25
    assert np.array_equal(sj["shift"], jt["shift"]) and np.array_equal(sj["scale"], jt["scale"])
    # targets: the product block first, then the exposure block; -1 where there is none
    assert sj["coeff_off"][:3].tolist() == [[1000 + 4 * K, -1], [0 + 1 * K, 1000 + 2 * K], [0, 1000]]
    assert sj["coeff_off"][6].tolist() == [1400 + 2 * K, -1]


def test_chain_rows_equal_the_step_major_rows():
    """every (product, date) system of the chain-major tables equals, field for field, the row the product-batched route's
    step-major table holds for it (the same job and solve records: what makes the two routes bit-equal on the device)"""
    jobs, x_range, reg_base, expo_base = _book()
    stateless, _rest, jt, sj, chain_begin, _w = C.lsm_date_chains(jobs, x_range, reg_base, expo_base, N_LOCAL, K)
    jt_s, sj_s, step_begin, step_states, S_of, w_len = C.lsm_step_tables(stateless, x_range, reg_base, expo_base, N_LOCAL, K)
    assert S_of == [1, 1, 1, 1] and step_states.tolist() == [1, 1, 1] and step_begin.tolist() == [0, 3, 5, 7] and w_len == 4 * N_LOCAL
    seen = 0
    for c, (p_i, _p, sched, _a) in enumerate(stateless):
        rows = np.nonzero(jt_s["product"] == p_i)[0]                   # ascending rows = ascending steps = schedule order
        assert len(rows) == len(sched) == chain_begin[c + 1] - chain_begin[c]
        for r, row in enumerate(rows):
            j = chain_begin[c] + r
            assert jt[j].tobytes() == jt_s[row].tobytes() and sj[j].tobytes() == sj_s[row].tobytes(), (c, r, jt[j], jt_s[row], sj[j], sj_s[row])
            seen += 1
    assert seen == len(jt) == len(jt_s)


def test_step_major_tables_of_a_mixed_book():
    """lsm_step_tables on the whole hand-made book (state counts 1, 2, 3): one step per (date index, state count), cache blocks
    of S rows behind each other"""
    jobs, x_range, reg_base, expo_base = _book()
    jt, sj, step_begin, step_states, S_of, w_len = C.lsm_step_tables(jobs, x_range, reg_base, expo_base, N_LOCAL, K)
    assert S_of == [1, 2, 1, 1, 1, 3] and w_len == 9 * N_LOCAL
    assert step_states.tolist() == [1, 2, 3, 1, 2, 3, 1] and step_begin.tolist() == [0, 3, 4, 5, 7, 8, 9, 11]
    assert jt["product"].tolist() == [0, 2, 4, 1, 5, 0, 2, 1, 5, 0, 2]
    w_of = {0: 0, 1: N_LOCAL, 2: 3 * N_LOCAL, 3: 4 * N_LOCAL, 4: 5 * N_LOCAL, 5: 6 * N_LOCAL}
    assert jt["w_offset"].tolist() == [w_of[p] for p in jt["product"].tolist()]
    assert sj["coeff_off"][3].tolist() == [100 + 1 * 2 * K, -1] and sj["coeff_off"][8].tolist() == [500, 1500 + 1 * 3 * K]


def test_symbols_flag_and_clone(oracle):
    for name in ("mcx_lsm_dates_moments", "mcx_lsm_dates_run"):
        assert name in _native._EXPORTS
        assert name + "(" in open(os.path.join(ROOT, "include", "mcx.h")).read()
    assert _abi.ABI_VERSION == 6
    assert hasattr(_native.HipBackend, "lsm_dates_moments") and hasattr(_native.HipBackend, "lsm_dates_run")
    sc, _ = cases.make_controller("irs_cva", oracle, inject=False)
    assert sc.date_batched_lsm is False
    assert sc.lsm_routes == {"dates": 0, "batched_steps": 0, "per_product": 0}
    for flag in (True, False):
        sc.date_batched_lsm = flag
        assert aad._clone_controller(sc, sc.model, True).date_batched_lsm is flag
    # a backend without the entry points keeps today's routes whatever the flag says
    sc.date_batched_lsm = True
    res_on = sc.run_simulation()
    assert sc.lsm_routes["dates"] == 0 and sc.lsm_routes["per_product"] == 1
    sc2, _ = cases.make_controller("irs_cva", oracle, inject=False)
    assert res_on.results == sc2.run_simulation().results
