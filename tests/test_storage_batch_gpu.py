"""The product-batched backward induction of gas storages (k6_step_batch / k6_finish_solve_batch behind mcx_storage_lsm_*_batch,
SimulationController._storage_regression_batched).  Every comparison is against the PER-STORAGE route (mcx_storage_lsm_run, one
call per storage) on the same book and the same paths, never against the batch itself, and it is bit for bit: a job's blocks run
the program text of k6_step on the tiling k6_step would get, and the fixed-order finish sums the same partials in the same order.
The per-storage route is pinned to the reference by tests/test_storage_gpu.py."""
import numpy as np
import pytest
import torch

import storage_cases
from emulated_ranks import run_ranks
from mcx import _abi
from mcx.controller.controller import storage_lsm_dates, storage_lsm_job_table

pytestmark = pytest.mark.gpu

# (n_states, end, rollout interval): schedules of different length, so late steps hold two jobs and then one.  S = 2 and 32 are the
# smallest and the largest state count (32 fills the LDS rows).  BIG: short schedules and S <= 7 for the largest path count.
BOOK = ((2, 8.0, 1.0), (7, 7.5, 2.0), (32, 3.0, 1.0))
BOOK_BIG = ((2, 3.0, 1.0), (7, 5.5, 2.0), (4, 1.0, 1.0))
N_GRID_STRIDE = 262144 + 257      # 4 n_cu tiles of 256 paths cover 262,144: the smallest count on the grid-stride loop, ragged tail


def three_storage_controller(backend, K, n_pre, n_main=256, specs=BOOK, timeline=(0.0, 1.0, 2.5)):
    """three storages on the gas model in ONE netting set; PV + EPE (exposure dates that are no action dates: steps without a roll)"""
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    from mcx.maths.regression import PolyomialRegression
    mod = storage_cases.mcx_classes()
    stores = []
    for j, (S, end, rollout) in enumerate(specs):
        p = storage_cases._daily_store(mod, S, end, [(0.0, end + 1.0, 0.0, 12.0)], rollout=rollout)
        p.name = f"store{j}"
        stores.append(p)
    rm = mod["RiskMetrics"]([mod["PVMetric"](), mod["EPEMetric"]()], exposure_timeline=np.array(timeline))
    sc = SimulationController([mod["NettingSet"](name="st", products=stores)], storage_cases._gas_model(mod), rm, n_main, n_pre, 2,
                              SimulationScheme.ANALYTICAL, False, regression_function=PolyomialRegression(degree=K - 1), backend=backend)
    sc.materialize = True
    return sc


class Book:
    """a controller that has run (pre-simulation paths, uploaded book, native storages) and the date tables of its storages"""

    def __init__(self, hip, K, n, specs, timeline):
        sc = three_storage_controller(hip, K, n, specs=specs, timeline=timeline)
        sc.run_simulation()
        self.sc, self.hip, self.K, self.n = sc, hip, K, n
        self.paths = sc.last_state["paths_pre"]
        assert self.paths.shape[2] == n
        self.ids = sorted(sc._storage_meta)
        self.S_of = [sc.products[i].get_num_states() for i in self.ids]
        self.handles = [sc._storage_handle(i) for i in self.ids]
        scheds = [sc._regression_schedule(i, sc.products[i]) for i in self.ids]
        atoms = [sc._regression_atoms(s, sc.products[i].asset_ids[0]) for i, s in zip(self.ids, scheds)]
        x_ids = sorted({x for a in atoms for _, x in a})
        mm = hip.lsm_stats(sc.book, x_ids, self.paths)
        x_range = {x: (mm[q, 0], mm[q, 1]) for q, x in enumerate(x_ids)}
        self.dates_of = [storage_lsm_dates(S, K, s, a, x_range, sc._reg_coeff_base[i], sc._expo_coeff_base[i])
                         for i, S, s, a in zip(self.ids, self.S_of, scheds, atoms)]
        self.jobs, self.step_begin, self.job_of, self.w_len = storage_lsm_job_table(self.dates_of, self.S_of, n)
        self.tab_begin = np.concatenate([[0], np.cumsum(np.asarray(self.S_of)[self.jobs["storage"]] * K)])
        self._single = {}

    def reset(self):
        self.hip.book_reset_coeffs(self.sc.book, self.sc._coeffs_at_upload)

    def single(self, flags):
        """the per-storage route, computed once per flag word and left unchanged: per storage (coefficients [L][S][K], status [L],
        the two cache halves), and the book's coefficient array afterwards"""
        if flags not in self._single:
            self.reset()
            out = []
            for st, S, dates in zip(self.handles, self.S_of, self.dates_of):
                W = self.hip.zeros(2, S, self.n)
                c, s = self.hip.storage_lsm_run(self.sc.book, st, dates, self.paths, W, flags=flags)
                out.append((c, s, W.cpu().numpy()))
            self._single[flags] = (out, self.hip.book_get_coeffs(self.sc.book).copy())
        return self._single[flags]

    def batch(self, flags):
        self.reset()
        W = self.hip.zeros(self.w_len)
        table, status = self.hip.storage_lsm_run_batch(self.sc.book, self.handles, self.jobs, self.step_begin, self.paths, W, self.n, flags=flags)
        return table, status, W.cpu().numpy(), self.hip.book_get_coeffs(self.sc.book).copy()

    def assert_batch_equals_single(self, flags):
        ref, ref_book = self.single(flags)
        table, status, W, book = self.batch(flags)
        assert len(status) == len(self.jobs) and len(table) == self.tab_begin[-1]
        base = 0
        for j, (c, s, W_ref) in enumerate(ref):
            SK = self.S_of[j] * self.K
            got_c = np.stack([table[self.tab_begin[k]:self.tab_begin[k] + SK].reshape(self.S_of[j], self.K) for k in self.job_of[j]])
            assert np.array_equal(got_c, c, equal_nan=True), (j, np.abs(got_c - c).max())
            assert np.array_equal(status[self.job_of[j]], s), (j, status[self.job_of[j]], s)
            assert np.array_equal(W[base:base + W_ref.size].reshape(W_ref.shape), W_ref, equal_nan=True), j
            base += W_ref.size
        assert np.array_equal(book, ref_book, equal_nan=True)
        return status


_BOOKS = {}


def book_of(hip, K, n):
    key = (K, n)
    if key not in _BOOKS:
        big = n >= N_GRID_STRIDE
        _BOOKS.clear()                                              # one book at a time on the device
        _BOOKS[key] = Book(hip, K, n, BOOK_BIG if big else BOOK, (0.0, 1.0) if big else (0.0, 1.0, 2.5))
    return _BOOKS[key]


# ---- 1. kernel level ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64_cache", "f32_cache"])
@pytest.mark.parametrize("n", [257, 1000, N_GRID_STRIDE])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6])
def test_run_batch_is_bit_equal_to_the_per_storage_runs(K, n, f32, hip):
    """257: a tile with one live lane; 1,000: ragged, the large books' own count; 262,401: the grid-stride loop with a ragged tail"""
    b = book_of(hip, K, n)
    L = [len(d) for d in b.dates_of]
    assert len(set(L)) == 3 and np.diff(b.step_begin).tolist()[-1] == 1 and 2 in np.diff(b.step_begin).tolist()     # 3, then 2, then 1 job
    assert b.S_of == [s[0] for s in (BOOK_BIG if n >= N_GRID_STRIDE else BOOK)]
    b.assert_batch_equals_single(_abi.LSM_F32_CACHE if f32 else 0)


# ---- 2. a step split over several launches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 1200])
def test_a_step_split_over_several_launches_changes_nothing(cap, hip, monkeypatch):
    """at 1,000 paths (4 tiles) and K = 3 the jobs of the first step need 4 * 8 * (11 + 26 + 101) = 4,416 bytes of partial sums:
    a cap of 1,200 bytes takes the first two in one launch and the third in another, a cap of 1 byte gives every job its own"""
    b = book_of(hip, 3, 1000)
    assert b.S_of == [2, 7, 32] and b.step_begin[1] == 3
    b.single(0)
    monkeypatch.setenv("MCX_STORAGE_BATCH_PARTIAL_BYTES", str(cap))
    b.assert_batch_equals_single(0)


# ---- 3. controller level ------------------------------------------------------------------------------------------------------------
def _run(sc, batch):
    sc.batch_storage_lsm = batch
    res = sc.run_simulation()
    return dict(route=sc.storage_lsm_route,
                prod=[p.regression_coeffs.numpy().copy() for p in sc.products if getattr(p, "is_storage", False)],
                expo=[sc.regression_coeffs[i].numpy().copy() for i in sorted(sc._storage_meta)],
                cfs=sc.last_state["cfs"].cpu().numpy(), ex=sc.last_state["expo"].cpu().numpy(),
                metrics=[[np.array(m, dtype=np.float64) for m in ns] for ns in res.results])


def _assert_same_run(a, b):
    for key in ("prod", "expo"):
        assert len(a[key]) == len(b[key]) >= 2
        for x, y in zip(a[key], b[key]):
            assert np.array_equal(x, y, equal_nan=True), (key, np.abs(x - y).max())
    assert np.array_equal(a["cfs"], b["cfs"], equal_nan=True) and np.array_equal(a["ex"], b["ex"], equal_nan=True)
    for ns_a, ns_b in zip(a["metrics"], b["metrics"]):
        for m_a, m_b in zip(ns_a, ns_b):
            assert np.array_equal(m_a, m_b, equal_nan=True), (m_a, m_b)          # values and MC errors


@pytest.mark.parametrize("case", ["storage_mixed", "three_storages"])
def test_controller_routes_agree_bit_for_bit(case, hip):
    def build():
        if case == "storage_mixed":          # two storages + a call, two netting sets, CVA + EPE + PV, Philox draws
            return storage_cases.make_controller("storage_mixed", hip, inject=False)[0]
        return three_storage_controller(hip, 3, 1000, n_main=1000)
    on, off = _run(build(), True), _run(build(), False)
    assert (on["route"], off["route"]) == ("batch", "single")
    _assert_same_run(on, off)


# ---- 4. status parity ---------------------------------------------------------------------------------------------------------------
def test_status_of_a_rank_deficient_system_is_the_per_storage_routes(hip):
    """two paths and K = 3: a Gram matrix of rank two that is not flagged degenerate.  Whatever the device solve reports for it, the
    batch reports the same, and the controller ends with the same coefficients on either route (through the host-solve fallback of
    the storages concerned if the status is non-zero)"""
    b = book_of(hip, 3, 2)
    assert not any(d["degenerate"][:-1].any() for d in b.dates_of)
    status = b.assert_batch_equals_single(0)
    print("status of the batch at two paths:", status.tolist())
    _BOOKS.clear()
    on = _run(three_storage_controller(hip, 3, 2, n_main=257), True)
    off = _run(three_storage_controller(hip, 3, 2, n_main=257), False)
    assert (on["route"], off["route"]) == ("batch", "single")
    _assert_same_run(on, off)


# ---- 5. bounds: host-side checks, nothing is launched -------------------------------------------------------------------------------
def _bad_tables(b):
    S, n = b.S_of, b.n
    first_roll = int(np.nonzero(b.jobs["roll_date"] >= 0)[0][0])
    same = b.jobs.copy(); same["w_new"][first_roll] = same["w_old"][first_roll]
    beyond = b.jobs.copy(); beyond["w_old"][0] = b.w_len - S[beyond["storage"][0]] * n + 1
    index = b.jobs.copy(); index["storage"][1] = len(S)
    twice = b.jobs.copy(); twice["storage"][1] = twice["storage"][0]
    return {"w_new == w_old": (same, first_roll), "w_old outside": (beyond, 0), "storage index out of range": (index, 1),
            "appears twice": (twice, 1)}                            # (table, the job that is wrong)


@pytest.mark.parametrize("what", ["w_new == w_old", "w_old outside", "storage index out of range", "appears twice"])
def test_bad_job_tables_are_refused_before_any_launch(what, hip):
    from mcx._native import McxError
    b = book_of(hip, 3, 1000)
    b.reset()
    before = hip.book_get_coeffs(b.sc.book).copy()
    W = hip.zeros(b.w_len)
    table, bad = _bad_tables(b)[what]
    with pytest.raises(McxError) as e:
        hip.storage_lsm_run_batch(b.sc.book, b.handles, table, b.step_begin, b.paths, W, b.n)
    msg = hip.lib.mcx_last_error(hip.h).decode()
    assert e.value.code == -2 and what in msg and "mcx_storage_lsm_run_batch" in msg, msg
    hip.synchronize()
    assert not W.any().item() and np.array_equal(hip.book_get_coeffs(b.sc.book), before)        # nothing ran
    # the step-wise entry point makes the same checks (on the step that holds the wrong job)
    t = int(np.searchsorted(b.step_begin, bad, side="right")) - 1
    with pytest.raises(McxError) as e:
        hip.storage_lsm_step_batch(b.sc.book, b.handles, table[b.step_begin[t]:b.step_begin[t + 1]], b.paths, W, b.n, (2 * b.K - 1) + 32 * b.K)
    assert e.value.code == -2 and what in hip.lib.mcx_last_error(hip.h).decode()
    hip.synchronize()
    assert not W.any().item()


@pytest.mark.parametrize("what", ["w_new == w_old", "w_old outside", "storage index out of range", "appears twice"])
def test_bad_job_tables_are_refused_by_the_stepwise_entry_points(what, hip):
    """the smallest book (K = 2, 257 paths): mcx_storage_lsm_step_batch refuses all four tables; mcx_storage_lsm_solve_batch, which
    receives neither paths nor cache, the two that concern it.  After each refusal the cache (filled with a sentinel), the moments,
    the table and the book's coefficients are what they were: nothing ran"""
    from mcx._native import McxError
    b = book_of(hip, 2, 257)
    b.reset()
    before = hip.book_get_coeffs(b.sc.book).copy()
    table, bad = _bad_tables(b)[what]
    t = int(np.searchsorted(b.step_begin, bad, side="right")) - 1
    step = np.ascontiguousarray(table[b.step_begin[t]:b.step_begin[t + 1]], dtype=_abi.STORAGE_LSM_JOB_DTYPE)
    stride = (2 * b.K - 1) + 32 * b.K
    W = hip.zeros(b.w_len).fill_(1.5)
    with pytest.raises(McxError) as e:
        hip.storage_lsm_step_batch(b.sc.book, b.handles, step, b.paths, W, b.n, stride)
    msg = hip.lib.mcx_last_error(hip.h).decode()
    assert e.value.code == -2 and what in msg and "mcx_storage_lsm_step_batch" in msg, msg
    hip.synchronize()
    assert (W == 1.5).all().item() and np.array_equal(hip.book_get_coeffs(b.sc.book), before)
    if what not in ("storage index out of range", "appears twice"):
        return
    # (the library directly: the wrapper sizes the table from the storage indices before it calls)
    mom = hip.zeros(len(step), stride).fill_(2.5)
    tab = hip.zeros(len(step) * 32 * b.K).fill_(3.5)
    status = hip.zeros(len(step), dtype=torch.int32).fill_(7)
    rc = hip.lib.mcx_storage_lsm_solve_batch(hip.h, b.sc.book.ptr, hip._storage_array(b.handles), len(b.handles), _abi.ptr(step), len(step),
                                             mom.data_ptr(), stride, tab.data_ptr(), status.data_ptr(), hip._stream())
    msg = hip.lib.mcx_last_error(hip.h).decode()
    assert rc == -2 and what in msg and "mcx_storage_lsm_solve_batch" in msg, msg
    hip.synchronize()
    assert (mom == 2.5).all().item() and (tab == 3.5).all().item() and (status == 7).all().item()
    assert (W == 1.5).all().item() and np.array_equal(hip.book_get_coeffs(b.sc.book), before)


# ---- 6. three emulated ranks --------------------------------------------------------------------------------------------------------
def test_three_emulated_ranks_one_collective_per_step(hip):
    """uneven split of 1,000 paths; tolerances of tests/test_storage_emulated_ranks.py (the ranks sum their moments in another
    order than one shard does); the ranks themselves are bit-equal; with L_j the schedule lengths the batch saves
    sum_j L_j - max_j L_j all-reduces: one collective per step instead of one per (storage, date)"""
    from mcx import _native

    def build(be, batch):
        sc = three_storage_controller(be, 3, 1000, n_main=1000)
        sc.materialize = False
        sc.batch_storage_lsm = batch
        return sc

    def results(res):
        return [[np.array(m, dtype=float) for m in ns] for ns in res.results]

    def coeffs_of(sc):
        return [p.regression_coeffs.numpy().copy() for p in sc.products] + [sc.regression_coeffs[i].numpy().copy() for i in sorted(sc._storage_meta)]

    single = build(hip, True)
    ref = results(single.run_simulation())
    ref_coeffs = coeffs_of(single)
    L = [len(single._regression_schedule(i, single.products[i])) for i in sorted(single._storage_meta)]

    def body(sc, rank):
        return results(sc.run_simulation()), coeffs_of(sc), sc.storage_lsm_route

    out, calls_on = run_ranks(3, lambda rank: build(_native.HipBackend(0), True), body)
    n_on = calls_on["all_reduce"]
    _, calls_off = run_ranks(3, lambda rank: build(_native.HipBackend(0), False), body)
    assert n_on == calls_off["all_reduce"] - (sum(L) - max(L)), (n_on, calls_off["all_reduce"], L)
    for rank, (got, coeffs, route) in enumerate(out):
        assert route == "batch"
        for c, c_ref in zip(coeffs, ref_coeffs):
            assert np.allclose(c, c_ref, rtol=1e-8, atol=1e-11 * np.abs(c_ref).max()), (rank, np.abs(c - c_ref).max())
        for ns_r, ns_g in zip(ref, got):
            for m_r, m_g in zip(ns_r, ns_g):
                assert np.allclose(m_r[:, 0], m_g[:, 0], rtol=1e-9, atol=1e-12), (rank, m_r[:, 0], m_g[:, 0])
    for got, coeffs, _ in out[1:]:
        for ns_a, ns_b in zip(out[0][0], got):
            for a, b_ in zip(ns_a, ns_b):
                assert np.array_equal(a, b_, equal_nan=True)
        for c_a, c_b in zip(out[0][1], coeffs):
            assert np.array_equal(c_a, c_b, equal_nan=True)
    torch.cuda.synchronize()
