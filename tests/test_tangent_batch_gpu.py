"""Product-batched forward-mode regression on the GPU (mcx_tangent_lsm_batch, csrc/kt_book.hip kt_lsm_batch; the routes of
SimulationController.batch_tangent_lsm in mcx/aad.py run_with_tangent_book).

  1. kernel level: every job of a batched call equals mcx_tangent_lsm for the same arguments BIT FOR BIT, at path counts that take
     one ragged block, two blocks, and a second grid-stride round, with a padded leading dimension, unsplit and one job per launch;
  2. refusals: a bad job anywhere in the table fails the call before anything runs;
  3. a 72-product book (more than the 64 of the per-job route) completes in forward mode and meets the reference's autograd;
  4. both routes give the same bits, and the default still takes the per-job route on small books;
  5. a storage book above 64 products completes; 6. three emulated ranks: one collective per parameter chunk."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import large_cva_cases
from mcx import _abi
from mcx.maths.regression import PolyomialRegression
from test_oracle_golden import check_lsm_sensitivities

pytestmark = pytest.mark.gpu
NP = _abi.TANGENT_NP
JOB = _abi.TANGENT_LSM_JOB_DTYPE


# ---- 1. kernel level -------------------------------------------------------------------------------------------------------------------
def _mixed_cva_book(hip, degree):
    ns, model, rm = cases.mixed_cva()
    sc = cases.SimulationController(ns, model, rm, 512, 512, 2, cases.E, backend=hip, regression_function=PolyomialRegression(degree=degree))
    sc.materialize = True
    sc.run_simulation()
    return sc


def _dual_inputs(sc, hip, n, ld, seed):
    """Philox dual paths of n paths in [T][D][ld] tensors whose columns >= n are NaN, random descriptor tangents, and the job table
    of every (stateless product, regression date) pair plus one job with an empty cash range"""
    from mcx.aad import stateless_lsm_jobs
    rng = np.random.default_rng(seed)
    plan = sc._sim.plan
    dslot = rng.normal(0.0, 0.05, (plan.n_slots, _abi.SLOT_NPARAM, NP))
    dinit = rng.normal(0.0, 0.05, (plan.n_state, NP))
    daux = rng.normal(0.0, 0.05, (plan.n_steps, plan.n_slots, _abi.AUX, NP))
    paths, dpaths = hip.tangent_paths(sc._sim, dslot, dinit, daux, 42, 0, n)
    h_datoms = rng.normal(0.0, 0.3, (len(sc.book_plan.atoms), 5, NP))
    h_datoms[:, 3:] *= 0.1                                                  # (tangents of the exponent's coefficients)
    datoms = hip.from_numpy(h_datoms)
    lsm_plan, _ = sc._regression_plan()
    x_ids = sorted({x for _, _, _, atoms in lsm_plan for _, x in atoms})
    stats = hip.lsm_stats(sc.book, x_ids, paths)
    x_range = {x: (stats[i, 0], stats[i, 1]) for i, x in enumerate(x_ids)}
    table, keep = stateless_lsm_jobs(lsm_plan, x_range, sc._expo_coeff_base, sc.book_plan.n_basis)
    swap = len(sc.products) - 1                                             # the unequal-tenor swap: cash terms with den >= 0
    assert (sc.book_plan.terms["den"] >= 0).any() and (table["product"] == swap).any()
    pr = sc.book_plan.products[swap]
    last = table[table["product"] == swap][-1].copy()
    last["first_event"] = pr["cf_end"] - pr["cf_begin"]                     # nothing left to pay: Y = 0
    table = np.concatenate([table, np.array([last], dtype=JOB)])
    if ld != n:
        wide, dwide = hip.empty(*paths.shape[:2], ld), hip.empty(NP, *paths.shape[:2], ld)
        wide.fill_(float("nan")); dwide.fill_(float("nan"))
        wide[..., :n] = paths; dwide[..., :n] = dpaths
        paths, dpaths = wide, dwide
    return table, datoms, paths, dpaths


def _check_bit_equality(sc, hip, monkeypatch, n, ld, seed):
    table, datoms, paths, dpaths = _dual_inputs(sc, hip, n, ld, seed)
    K = sc.book_plan.n_basis
    single = np.stack([hip.tangent_lsm(sc.book, int(j["product"]), int(j["first_event"]), int(j["num_atom"]), int(j["x_atom"]),
                                       float(j["shift"]), float(j["scale"]), datoms, paths, dpaths, n_paths=n) for j in table])
    assert single.shape == (len(table), 1 + NP, 3 * K - 1) and not np.isnan(single).any()
    assert np.all(single[:, 0, 0] == n)                                     # sum of z^0
    assert np.all(single[-1, :, 2 * K - 1:] == 0.0) and np.abs(single[:-1, :, 2 * K - 1:]).max() > 0.0
    for var in (None, "1"):                                                 # unsplit; one job per launch
        if var is None:
            monkeypatch.delenv("MCX_TANGENT_BATCH_PARTIAL_BYTES", raising=False)
        else:
            monkeypatch.setenv("MCX_TANGENT_BATCH_PARTIAL_BYTES", var)
        batch = hip.tangent_lsm_batch(sc.book, table, datoms, paths, dpaths, n_paths=n)
        assert not np.isnan(batch).any()
        for j in range(len(table)):
            assert np.array_equal(batch[j], single[j]), (n, ld, var, j, np.abs(batch[j] - single[j]).max())
    return len(table)


@pytest.fixture(scope="module")
def mixed_books(hip):
    return {}


def _book(mixed_books, hip, degree):
    if degree not in mixed_books:
        mixed_books[degree] = _mixed_cva_book(hip, degree)
    return mixed_books[degree]


def _path_counts(hip):
    tiles = 2 * hip.device_info()["n_cu"]
    return [(1, 1), (63, 63), (300, 300), (256 * tiles + 257, 256 * tiles + 257 + 37)]


@pytest.mark.parametrize("which", range(4), ids=["n1", "n63", "n300", "second_round_padded_ld"])
def test_batch_equals_the_single_call_bit_for_bit(which, hip, mixed_books, monkeypatch):
    n, ld = _path_counts(hip)[which]
    n_jobs = _check_bit_equality(_book(mixed_books, hip, 2), hip, monkeypatch, n, ld, 100 + which)
    assert n_jobs >= 9


@pytest.mark.parametrize("degree", [0, 1, 3])
def test_batch_equals_the_single_call_at_every_basis_size(degree, hip, mixed_books, monkeypatch):
    sc = _book(mixed_books, hip, degree)
    assert sc.book_plan.n_basis == degree + 1
    _check_bit_equality(sc, hip, monkeypatch, 300, 300, 200 + degree)


def test_empty_table_and_no_paths(hip, mixed_books):
    sc = _book(mixed_books, hip, 2)
    table, datoms, paths, dpaths = _dual_inputs(sc, hip, 63, 63, 7)
    assert hip.tangent_lsm_batch(sc.book, table[:0], datoms, paths, dpaths).shape == (0, 1 + NP, 8)
    out = np.full((len(table), 1 + NP, 8), np.nan)
    hip.tangent_lsm_batch(sc.book, table, datoms, paths, dpaths, n_paths=0, out=out)
    assert np.all(out == 0.0)


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------------
def _refused(hip, sc, table, datoms, paths, dpaths, code, what):
    from mcx._native import McxError
    K = sc.book_plan.n_basis
    out = np.full((len(table), 1 + NP, 3 * K - 1), np.nan)
    with pytest.raises(McxError) as e:
        hip.tangent_lsm_batch(sc.book, table, datoms, paths, dpaths, out=out)
    assert e.value.code == code and what in str(e.value) and "mcx_tangent_lsm_batch" in str(e.value), str(e.value)
    assert np.isnan(out).all(), "h_moments written by a refused call"


def test_refusals_on_the_mixed_book(hip, mixed_books):
    sc = _book(mixed_books, hip, 2)
    table, datoms, paths, dpaths = _dual_inputs(sc, hip, 300, 300, 9)
    good = table[:1]
    pr = sc.book_plan.products[int(good[0]["product"])]

    def bad(**kw):
        j = good.copy()
        for k, v in kw.items():
            j[0][k] = v
        return np.concatenate([good, j, good])

    _refused(hip, sc, bad(product=len(sc.products)), datoms, paths, dpaths, -2, "product out of range")
    _refused(hip, sc, bad(first_event=pr["cf_end"] - pr["cf_begin"] + 1), datoms, paths, dpaths, -2, "first_event out of range")
    _refused(hip, sc, bad(x_atom=len(sc.book_plan.atoms)), datoms, paths, dpaths, -2, "atom out of range")
    # ld < n_paths (the Python wrapper cannot say that: the library is called as a C caller would)
    out = np.full((1, 1 + NP, 8), np.nan)
    rc = hip.lib.mcx_tangent_lsm_batch(hip.h, sc.book.ptr, _abi.ptr(good), C.c_int32(1), C.c_void_p(datoms.data_ptr()),
                                       C.c_void_p(paths.data_ptr()), C.c_void_p(dpaths.data_ptr()), C.c_int64(300), C.c_int64(299),
                                       C.c_int32(paths.shape[0]), _abi.ptr(out), hip._stream())
    assert rc == -2 and np.isnan(out).all()
    # and the table is fine
    assert not np.isnan(hip.tangent_lsm_batch(sc.book, bad(), datoms, paths, dpaths)).any()


def _any_inputs(sc, hip):
    paths = sc.last_state["paths"].contiguous()
    return hip.zeros(len(sc.book_plan.atoms), 5, NP), paths, hip.zeros(NP, *paths.shape)


def test_a_product_with_exercise_states_is_refused(hip):
    ns, model, rm = cases.bermudan_swaption()
    bond = cases.Bond(0.0, 2.0, 1.0, 0.5, True, 0.03)
    ns = [cases.NettingSet(name="berm_ns", products=[bond] + list(ns[0].products))]
    sc = cases.SimulationController(ns, model, rm, 256, 256, 1, cases.E, backend=hip)
    sc.materialize = True
    sc.run_simulation()
    assert [int(s) for s in sc.book_plan.products["n_states"]][0] == 1 and sc.book_plan.products["n_states"][1] > 1
    table = np.array([(0, 0, 0, 0, 0.0, 1.0), (1, 0, 0, 0, 0.0, 1.0)], dtype=JOB)
    _refused(hip, sc, table, *_any_inputs(sc, hip), _abi.E_NOT_FUSABLE, "stateless products only")
    assert not np.isnan(hip.tangent_lsm_batch(sc.book, table[:1], *_any_inputs(sc, hip))).any()


def test_a_basket_mode_option_event_is_refused(hip):
    ns, model, rm = cases.basket_model_config()
    call = cases.EuropeanOption(cases.Equity("asset1"), 1.0, 100.0, cases.OptionType.CALL, asset_id="asset1")
    ns = [cases.NettingSet(name="plain", products=[call])] + ns
    sc = cases.SimulationController(ns, model, rm, 256, 0, 2, cases.E, backend=hip)
    sc.materialize = True
    sc.run_simulation()
    ev, pr = sc.book_plan.events, sc.book_plan.products
    basket = [p for p in range(len(pr)) if any(ev["kind"][q] == _abi.EV_OPTION and ev["aux"][q][0] != 0.0
                                               for q in range(pr["cf_begin"][p], pr["cf_end"][p]))]
    assert basket and 0 not in basket and sc.book_plan.n_basis <= 4
    table = np.array([(0, 0, 0, 0, 0.0, 1.0), (basket[0], 0, 0, 0, 0.0, 1.0)], dtype=JOB)
    _refused(hip, sc, table, *_any_inputs(sc, hip), _abi.E_NOT_FUSABLE, "has no tangent form")


# ---- 3. the capability ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large_batched(hip):
    sc, g = large_cva_cases.make_controller(hip)
    return sc, g, sc.run_simulation()


def _same(a, b):
    """results and derivatives [netting set][metric][evaluation] of two runs, bit for bit"""
    flat = lambda nested: [np.array(m, dtype=np.float64) for ns in nested for m in ns]
    return all(len(x) == len(y) and all(u.shape == v.shape and np.array_equal(u, v) for u, v in zip(x, y))
               for x, y in ((flat(a.results), flat(b.results)), (flat(a.derivatives), flat(b.derivatives))))


def test_a_book_of_72_products_runs_in_forward_mode(large_batched):
    """fails without the feature: the book went to bump-and-revalue (timings["tangent"] False)"""
    sc, g, res = large_batched
    assert len(sc.products) == 72 and sc.batch_tangent_lsm is None
    assert sc.timings["tangent"] is True and sc.timings["batched_lsm_jobs"] > 0 and sc.timings["forward_mode_passes"] == 3, sc.timings
    check_lsm_sensitivities(sc, g, res)


# ---- 4. route equality, unchanged default ------------------------------------------------------------------------------------------------
def test_routes_agree_bit_for_bit_and_the_default_is_unchanged(hip, large_batched, monkeypatch):
    calls, tables = [], []
    single, batch = hip.tangent_lsm, hip.tangent_lsm_batch

    def rec_single(book, product, first, num, x, shift, scale, *a, **k):
        calls.append((product, first, num, x, shift, scale))
        return single(book, product, first, num, x, shift, scale, *a, **k)

    def rec_batch(book, jobs, *a, **k):
        tables.append(np.array(jobs, dtype=JOB))
        return batch(book, jobs, *a, **k)
    monkeypatch.setattr(hip, "tangent_lsm", rec_single, raising=False)
    monkeypatch.setattr(hip, "tangent_lsm_batch", rec_batch, raising=False)

    sc, _ = cases.make_controller("mixed_cva_aad", hip)
    default = sc.run_simulation()
    assert sc.timings["tangent"] is True and sc.timings["batched_lsm_jobs"] == 0 and calls and not tables
    per_job_calls = list(calls)
    sc, _ = cases.make_controller("mixed_cva_aad", hip)
    sc.batch_tangent_lsm = True
    batched = sc.run_simulation()
    assert sc.timings["batched_lsm_jobs"] == len(per_job_calls) and len(tables) == sc.timings["forward_mode_passes"]
    assert calls == per_job_calls, "the batched route made per-job calls"
    assert [tuple(r) for t in tables for r in t.tolist()] == per_job_calls     # the job tables: the per-job loop's arguments, in its order
    assert _same(default, batched)

    sc, _ = large_cva_cases.make_controller(hip)
    sc.batch_tangent_lsm = False
    del calls[:], tables[:]
    per_job = sc.run_simulation()
    assert sc.timings["tangent"] is True and sc.timings["batched_lsm_jobs"] == 0 and not tables
    assert len(calls) == large_batched[0].timings["batched_lsm_jobs"]
    assert _same(per_job, large_batched[2])


# ---- 5. a storage book above the cap -------------------------------------------------------------------------------------------------
def test_storage_book_of_67_products_completes_in_forward_mode(hip):
    """fails without the feature: NotImplementedError (a book that holds a storage is never bumped)"""
    import storage_cases
    from test_storage_aad_gpu import controller, gradients
    from test_storage_aad_reference import check_against_reference, load_aad

    def with_fill(mod):
        ns, model, rm = storage_cases.storage_mixed(mod)
        calls = []
        for k in range(64):
            c = mod["EuropeanOption"](mod["Equity"]("a1"), 1.0, 80.0 + k, mod["OptionType"].CALL, asset_id="a1")
            c.name = f"fill_call_{k}"
            calls.append(c)
        return ns + [mod["NettingSet"](name="fill", products=calls, counterparty_id="cp")], model, rm

    two = controller("storage_mixed", hip, True)
    ref = gradients(two.run_simulation())
    sc = controller("storage_mixed", hip, True, build=with_fill)
    res = sc.run_simulation()
    assert len(sc.products) == 67
    assert torch.equal(sc.simulation_timeline, two.simulation_timeline)      # the fixture's draws still fit
    assert sc.timings["tangent"] is True and "batched_lsm_jobs" in sc.timings, sc.timings
    print("batched jobs of the storage book:", sc.timings["batched_lsm_jobs"])
    got = gradients(res)
    ga = load_aad("storage_mixed")
    worst = 0.0
    for ns_i in range(2):
        for m_i, m in enumerate(sc.risk_metrics.metrics):
            check_against_reference("storage_mixed+fill", ga, f"{ns_i}_{m_i}", got[ns_i][m_i], m.get_name() == "pv")
            scale = np.abs(ref[ns_i][m_i]).max(axis=1, keepdims=True)
            worst = max(worst, float((np.abs(got[ns_i][m_i] - ref[ns_i][m_i]) / np.maximum(scale, 1e-300)).max()))
    print("storage_mixed + 64 calls against the two-set run: max gradient difference / max|row|", worst)
    assert all(np.isfinite(g).all() for g in got[2])


# ---- 6. three emulated ranks ---------------------------------------------------------------------------------------------------------
class _RecordingShard:
    def __init__(self, inner, shapes):
        self._inner, self._shapes = inner, shapes

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def all_reduce_np(self, a):
        if self._inner.rank == 0:
            self._shapes.append(tuple(np.shape(a)))
        return self._inner.all_reduce_np(a)


def test_72_products_on_three_emulated_ranks(hip):
    from emulated_ranks import run_ranks
    from mcx import _native

    def build(be):
        sc, _ = large_cva_cases.make_controller(be, inject=False)
        sc.materialize = False
        return sc

    grads = lambda res: [[np.array(m, dtype=np.float64) for m in ns] for ns in res.derivatives]
    one = build(hip)
    ref = grads(one.run_simulation())
    n_jobs, passes = one.timings["batched_lsm_jobs"], one.timings["forward_mode_passes"]
    shapes = []

    def body(sc, rank):
        inner = sc.shard_factory
        sc.shard_factory = lambda: _RecordingShard(inner(), shapes)
        return grads(sc.run_simulation())

    out, calls = run_ranks(3, lambda rank: build(_native.HipBackend(0)), body)
    K = one.regression_function.get_degree()                                # (the number of basis functions)
    block = (1 + NP, 3 * K - 1)
    assert [s for s in shapes if s[-2:] == block] == [(n_jobs // passes,) + block] * passes, shapes     # one collective per chunk
    for rank, got in enumerate(out):
        for ns_r, ns_g in zip(ref, got):
            for m_r, m_g in zip(ns_r, ns_g):
                scale = np.abs(m_r).max(axis=1, keepdims=True)
                print("rank", rank, "max gradient difference / max|row|", (np.abs(m_r - m_g) / np.maximum(scale, 1e-300)).max())
                assert np.allclose(m_r, m_g, rtol=1e-9, atol=1e-12), (rank, m_r, m_g)
