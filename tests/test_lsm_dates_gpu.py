"""Date-batched LSM (k3_dates behind mcx_lsm_dates_moments / mcx_lsm_dates_run; SimulationController.date_batched_lsm).

Kernel and entry level
  1. bit equality with the product-batched route: for the same job and solve records the moments of every system, the rolled cache
     and the book's coefficients equal those of mcx_lsm_step_batch_dev / mcx_lsm_run_batch issued step by step in schedule order;
  2. a chain of length one, a table of one chain, two launches split by the chain limit, n_paths = 0, every refusal;
  3. the moments against the long-double reference under the bound of tests/test_lsm_basis_sizes.py:
     |m - m_ref| <= C_MOM (2K + log2 n) eps sum|term|, on the kernel's own rolled cache.
Controller level: flag on against flag off (bitwise where the off route has the same tiling), the reference fixtures, the mixed
book, forward mode and the singular fallback."""
import math

import numpy as np
import pytest
import torch

import cases
import lsm_reference as R
from mcx import _abi
from mcx._native import McxError
from mcx.controller import controller as C
from mcx.maths.regression import PolyomialRegression

pytestmark = pytest.mark.gpu

C_MOM = 4.0                                    # tests/test_lsm_basis_sizes.py
PATH_COUNTS = (1, 63, 257, 4097, 20011)        # one lane, under one wave, a ragged second block, 17 blocks, the 64-block cap
BASIS = (1, 2, 3, 4, 6)


def _bs_payoffs():
    """a European, a binary and a Brownian-bridge barrier option on Black-Scholes with exposure dates (ENE keeps the European on the
    regression): the payoff branches of k3_cash_event and the bridge counters"""
    model = cases.BlackScholesModel(0, 100.0, 0.03, 0.25)
    eu = cases.EuropeanOption(cases.Equity(), 1.0, 95.0, cases.OptionType.CALL)
    bi = cases.BinaryOption(1.0, 100.5, 10.0, cases.OptionType.CALL)
    ba = cases.BarrierOption(0.0, 1.0, 100.0, 6, cases.OptionType.CALL, 125.0, cases.BarrierOptionType.UPANDOUT)
    ba.set_use_brownian_bridge()
    for k, p in enumerate((eu, bi, ba)):
        p.name = f"p{k}"
    rm = cases.RiskMetrics([cases.EPEMetric(), cases.ENEMetric()], exposure_timeline=np.array([0.0, 0.25, 0.5, 0.75, 1.0]))
    return [cases.NettingSet(name=p.name, products=[p]) for p in (eu, bi, ba)], model, rm


BOOKS = {"irs_cva": (cases.irs_cva, 2, cases.E), "netting": (cases.netting, 1, cases.A), "mixed_cva": (cases.mixed_cva, 2, cases.E),
         "bs_payoffs": (_bs_payoffs, 2, cases.A)}


class _Book:
    """one compiled book at basis size K: the uploaded HIP book and its stateless regression jobs"""

    def __init__(self, hip, name, K):
        build, steps, scheme = BOOKS[name]
        ns, model, rm = build()
        sc = cases.SimulationController(ns, model, rm, 256, 256, steps, scheme, backend=hip, regression_function=PolyomialRegression(degree=K - 1))
        sc.prepare()
        sc._set_bridge_rng(43, 0, "bridge_pre")
        self.hip, self.sc, self.book, self.K, self.NM = hip, sc, sc.book, K, (2 * K - 1) + K
        assert sc.book_plan.n_basis == K
        self.plan, storage = sc._regression_plan()
        assert self.plan and not storage and all(p.get_num_states() == 1 for _, p, _, _ in self.plan), name
        self.coeffs0 = hip.book_get_coeffs(self.book).copy()

    def paths(self, n, pad=0, seed=11):
        """[T][D][n] pre-simulation paths, rows `pad` doubles apart beyond n"""
        p = self.hip.generate_paths(self.sc._sim, seed, 0, n)
        if pad == 0:
            return p
        wide = self.hip.zeros(p.shape[0], p.shape[1], n + pad).fill_(float("nan"))
        wide[:, :, :n] = p
        return wide[:, :, :n]

    def tables(self, paths, ld_w):
        """chain-major tables and the step-major tables of the same systems (caches of ld_w doubles per product), plus `rows`: the
        step-major row of every chain-major row"""
        sc = self.sc
        xr = sc._explanatory_ranges(sc._shard, self.plan, paths)
        args = (xr, sc._reg_coeff_base, sc._expo_coeff_base, ld_w, self.K)
        stateless, rest, jt, sj, cb, w_len = C.lsm_date_chains(self.plan, *args)
        assert not rest and len(jt) == sum(len(s) for _, _, s, _ in self.plan)
        jt_s, sj_s, step_begin, step_states, _S, w_len_s = C.lsm_step_tables(stateless, *args)
        assert w_len_s == w_len and (step_states == 1).all()
        rows = np.zeros(len(jt), dtype=np.int64)
        for c, (p_i, _p, sched, _a) in enumerate(stateless):
            rows[cb[c]:cb[c + 1]] = np.nonzero(jt_s["product"] == p_i)[0]
        assert jt[np.arange(len(jt))].tobytes() == jt_s[rows].tobytes() and sj.tobytes() == sj_s[rows].tobytes()
        return dict(jt=jt, sj=sj, cb=cb, w_len=w_len, jt_s=jt_s, sj_s=sj_s, step_begin=step_begin, step_states=step_states, rows=rows)

    def reset(self):
        self.hip.book_reset_coeffs(self.book, self.coeffs0)

    def batched_moments(self, t, paths, ld_w, flags):
        """the product-batched route step by step in schedule order -> (moments [n_jobs][NM] in chain-major order, the cache)"""
        W = self.hip.zeros(t["w_len"])
        mom = np.zeros((len(t["jt_s"]), self.NM))
        for s_ in range(len(t["step_states"])):
            j0, j1 = int(t["step_begin"][s_]), int(t["step_begin"][s_ + 1])
            mom[j0:j1] = self.hip.lsm_step_batch_dev(self.book, t["jt_s"][j0:j1], 1, paths, W, ld_w, flags=flags).cpu().numpy()
        return mom[t["rows"]], W


_BOOKS = {}


@pytest.fixture(scope="module")
def books(hip):
    def get(name, K):
        if (name, K) not in _BOOKS:
            _BOOKS[(name, K)] = _Book(hip, name, K)
        return _BOOKS[(name, K)]
    yield get
    _BOOKS.clear()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. bit equality with the product-batched route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", BASIS)
@pytest.mark.parametrize("name", list(BOOKS))
def test_moments_cache_and_coefficients_equal_the_batched_route(name, K, books, hip):
    """every path count, float32 cache quirk on and off, padded leading dimensions of the paths and of the cache at every count but
    4097 (ld = n + 3, ld_w = n + 5)"""
    b = books(name, K)
    for n in PATH_COUNTS:
        pad, pad_w = (0, 0) if n == 4097 else (3, 5)
        paths, ld_w = b.paths(n, pad), n + pad_w
        t = b.tables(paths, ld_w)
        for flags in (0, _abi.LSM_F32_CACHE):
            tag = (name, K, n, flags)
            ref, W_ref = b.batched_moments(t, paths, ld_w, flags)
            W = hip.zeros(t["w_len"])
            mom = hip.lsm_dates_moments(b.book, t["jt"], t["cb"], paths, W, ld_w, flags=flags).cpu().numpy()
            assert mom.shape == ref.shape and np.isfinite(ref).all(), tag
            assert np.array_equal(_bits(mom), _bits(ref)), (tag, np.nonzero((_bits(mom) != _bits(ref)).any(axis=1))[0])
            assert torch.equal(W, W_ref), tag
            assert ref[:, 0].tolist() == [float(n)] * len(ref), tag                     # sum z^0 = n: every system saw every path once
            # the one-call inductions: coefficients, flag and cache
            b.reset()
            W1 = hip.zeros(t["w_len"])
            f1 = hip.lsm_run_batch(b.book, t["jt_s"], t["sj_s"], t["step_begin"], t["step_states"], paths, W1, ld_w, flags=flags)
            c1 = hip.book_get_coeffs(b.book).copy()
            b.reset()
            W2 = hip.zeros(t["w_len"])
            f2 = hip.lsm_dates_run(b.book, t["jt"], t["sj"], t["cb"], paths, W2, ld_w, flags=flags)
            c2 = hip.book_get_coeffs(b.book).copy()
            assert f1 == f2 and np.array_equal(_bits(c1), _bits(c2)), (tag, f1, f2, np.abs(c1 - c2).max())
            assert torch.equal(W1, W_ref) and torch.equal(W2, W_ref), tag
            if n >= 4097 and K <= 3:
                assert f2 == 0, tag
            assert f2 != 0 or not np.array_equal(c2, b.coeffs0), tag                      # (a singular system writes no coefficients)
    b.reset()


def test_chain_of_one_job_and_table_of_one_chain(books, hip):
    b = books("irs_cva", 3)
    n = 257
    paths = b.paths(n)
    t = b.tables(paths, n)
    assert len(t["cb"]) == 2                                                             # irs_cva: one product, one chain
    j = int(np.argmax(t["jt"]["roll_end"] - t["jt"]["roll_begin"]))                     # (the widest roll window: the cache moves)
    job = t["jt"][j:j + 1]
    W_ref, W = hip.zeros(n), hip.zeros(n)
    ref = hip.lsm_step_batch(b.book, job, 1, paths, W_ref, n)
    mom = hip.lsm_dates_moments(b.book, job, np.array([0, 1]), paths, W, n).cpu().numpy()
    assert np.array_equal(_bits(mom), _bits(ref)) and torch.equal(W, W_ref) and W.any().item()
    # two chains of one job each on the same cache row are two independent launches' worth of work on distinct rows
    W2 = hip.zeros(2 * n)
    jobs2 = np.concatenate([job, job])
    jobs2["w_offset"][1] = n
    mom2 = hip.lsm_dates_moments(b.book, jobs2, np.array([0, 1, 2]), paths, W2, n).cpu().numpy()
    assert np.array_equal(_bits(mom2[0]), _bits(ref[0])) and np.array_equal(_bits(mom2[1]), _bits(ref[0]))
    assert torch.equal(W2[:n], W_ref) and torch.equal(W2[n:], W_ref)


def test_launches_split_by_the_chain_limit_give_the_bytes_of_one_launch(books, hip):
    """netting: four chains in one launch, in four launches of one chain, in launches of three + one and of two + two"""
    b = books("netting", 3)
    n = 4097
    paths = b.paths(n)
    t = b.tables(paths, n)
    assert len(t["cb"]) == 5
    W0 = hip.zeros(t["w_len"])
    m0 = hip.lsm_dates_moments(b.book, t["jt"], t["cb"], paths, W0, n).cpu().numpy()
    for limit in (1, 3):
        W = hip.zeros(t["w_len"])
        m = hip.lsm_dates_moments(b.book, t["jt"], t["cb"], paths, W, n, max_chains=limit).cpu().numpy()
        assert np.array_equal(_bits(m), _bits(m0)) and torch.equal(W, W0), limit
    coeffs = []
    for limit in (0, 2):
        b.reset()
        W = hip.zeros(t["w_len"])
        assert hip.lsm_dates_run(b.book, t["jt"], t["sj"], t["cb"], paths, W, n, max_chains=limit) == 0
        assert torch.equal(W, W0), limit
        coeffs.append(hip.book_get_coeffs(b.book).copy())
    assert np.array_equal(_bits(coeffs[0]), _bits(coeffs[1])) and not np.array_equal(coeffs[0], b.coeffs0)
    b.reset()


class _View:
    """the buffer and the strides of a paths tensor under another path count: n = 0 (an empty torch tensor has no data pointer,
    and the library rejects null pointers before it looks at the path count), or n above the row stride (a refusal)"""

    def __init__(self, t, n):
        self.t, self.shape = t, (t.shape[0], t.shape[1], n)

    def data_ptr(self):
        return self.t.data_ptr()

    def stride(self, k=None):
        return self.t.stride() if k is None else self.t.stride(k)

    def dim(self):
        return 3


def test_no_paths_gives_zero_moments_and_touches_nothing(books, hip):
    b = books("netting", 3)
    one = b.paths(1)
    t = b.tables(one, 1)
    W = hip.zeros(t["w_len"]).fill_(1.5)
    mom = hip.lsm_dates_moments(b.book, t["jt"], t["cb"], _View(one, 0), W, 1)
    assert mom.shape == (len(t["jt"]), b.NM) and not mom.any().item()
    assert (W == 1.5).all().item()
    # the one-call form solves the zero systems as the product-batched one does: same flag, same coefficients, cache untouched
    b.reset()
    f1 = hip.lsm_run_batch(b.book, t["jt_s"], t["sj_s"], t["step_begin"], t["step_states"], _View(one, 0), W, 1)
    c1 = hip.book_get_coeffs(b.book).copy()
    b.reset()
    f2 = hip.lsm_dates_run(b.book, t["jt"], t["sj"], t["cb"], _View(one, 0), W, 1)
    c2 = hip.book_get_coeffs(b.book).copy()
    assert f1 == f2 and np.array_equal(_bits(c1), _bits(c2)) and (W == 1.5).all().item()
    b.reset()


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_tables_before_any_launch(books, hip):
    """the pattern of tests/test_lsm_batch_entries.py on the netting book (four products of one state): after each refusal the cache
    (filled with a sentinel) and the book's coefficients are what they were (the flag of mcx_lsm_dates_run is a host word that the
    wrapper does not return when the call fails; mcx_lsm_dates_moments takes none)"""
    b = books("netting", 3)
    sc, plan, K = b.sc, b.sc.book_plan, b.K
    n = 1024
    paths = b.paths(n)
    W = hip.zeros(2 * n).fill_(1.5)
    before = hip.book_get_coeffs(b.book).copy()

    def tables(n_jobs=2):
        jobs = np.zeros(n_jobs, dtype=_abi.LSM_JOB_DTYPE)
        sj = np.zeros(n_jobs, dtype=_abi.LSM_SOLVE_JOB_DTYPE)
        sj["coeff_off"][:] = -1
        sj["scale"] = 1.0
        return jobs, sj

    def refused(jobs, sj, cb, words, code=-2, flags=0, pth=paths, ld_w=n):
        for who, call in (("mcx_lsm_dates_moments", lambda: hip.lsm_dates_moments(b.book, jobs, cb, pth, W, ld_w, flags=flags)),
                          ("mcx_lsm_dates_run", lambda: hip.lsm_dates_run(b.book, jobs, sj, cb, pth, W, ld_w, flags=flags))):
            with pytest.raises(McxError) as e:
                call()
            msg = hip.lib.mcx_last_error(hip.h).decode()
            assert e.value.code == code and words in msg and who in msg, (words, who, e.value.code, msg)
            hip.synchronize()
            assert (W == 1.5).all().item(), (words, who)
            assert np.array_equal(hip.book_get_coeffs(b.book), before), (words, who)

    one_chain = np.array([0, 2])
    # every index k3_check_job checks (in the second job of the chain: the first one is fine)
    for words, field, value in (("product out of range", "product", len(plan.products)), ("product out of range", "product", -1),
                                ("roll window", "roll_end", 10 ** 6), ("roll window", "roll_begin", -1),
                                ("atoms", "num_atom", len(plan.atoms)), ("atoms", "x_atom", -1),
                                ("outside d_W", "w_offset", n + 1), ("outside d_W", "w_offset", -1)):
        jobs, sj = tables()
        jobs[field][1] = value
        refused(jobs, sj, one_chain, words)
    # a product of more than one exercise state has no date-batched form
    sb, _ = cases.make_controller("american_put", hip, inject=False)
    sb.prepare()
    jobs, sj = tables(1)
    for who, call in (("mcx_lsm_dates_moments", lambda: hip.lsm_dates_moments(sb.book, jobs, np.array([0, 1]), paths, W, n)),
                      ("mcx_lsm_dates_run", lambda: hip.lsm_dates_run(sb.book, jobs, sj, np.array([0, 1]), paths, W, n))):
        with pytest.raises(McxError) as e:
            call()
        msg = hip.lib.mcx_last_error(hip.h).decode()
        assert e.value.code == -2 and "states" in msg and who in msg, msg
        hip.synchronize()
        assert (W == 1.5).all().item()
    # a chain whose jobs differ in w_offset (two valid cache rows) or in product
    jobs, sj = tables()
    jobs["w_offset"][1] = n
    refused(jobs, sj, one_chain, "differs from its chain")
    assert len(plan.products) == 4
    jobs, sj = tables()
    jobs["product"][1] = 1
    refused(jobs, sj, one_chain, "differs from its chain")
    # the chain table
    jobs, sj = tables()
    refused(jobs, sj, np.array([1, 2]), "must start at job 0")
    refused(jobs, sj, np.array([0, 2, 1, 2]), "not ascending")
    refused(jobs, sj, np.array([0, 1]), "must end at n_jobs")
    refused(jobs, sj, np.array([0, 1, 3]), "must end at n_jobs")
    # leading dimensions below the path count: of the cache, of the paths
    refused(jobs, sj, one_chain, "leading dimension", ld_w=n - 1)
    refused(jobs, sj, one_chain, "leading dimension", pth=_View(paths, n + 1), ld_w=n + 1)
    # no MFMA form
    refused(jobs, sj, one_chain, "MFMA", code=-3, flags=_abi.LSM_MFMA)
    # a [1][K] coefficient block that ends beyond the array, in either slot (the solve table: mcx_lsm_dates_run only)
    for slot in (0, 1):
        jobs, sj = tables()
        sj["coeff_off"][1, slot] = len(plan.coeffs) - K + 1
        with pytest.raises(McxError) as e:
            hip.lsm_dates_run(b.book, jobs, sj, one_chain, paths, W, n)
        msg = hip.lib.mcx_last_error(hip.h).decode()
        assert e.value.code == -2 and "coefficient offset" in msg and "mcx_lsm_dates_run" in msg, msg
        hip.synchronize()
        assert (W == 1.5).all().item() and np.array_equal(hip.book_get_coeffs(b.book), before)
    # the valid table runs
    jobs, sj = tables()
    assert hip.lsm_dates_moments(b.book, jobs, one_chain, paths, W, n).shape == (2, b.NM)


# ---- 3. the moments against the long-double reference ---------------------------------------------------------------------------------------
def test_moments_against_the_long_double_reference(books, hip):
    """irs_cva at 20011 paths (the 64-block cap, more than one path per lane).  The cache a system's moments were formed on is the
    cache after a run of the chain truncated behind that system: the kernel's own roll, date by date."""
    b = books("irs_cva", 3)
    n, K = 20011, b.K
    paths = b.paths(n)
    t = b.tables(paths, n)
    jt, L = t["jt"], len(t["jt"])
    W = hip.zeros(n)
    mom = hip.lsm_dates_moments(b.book, jt, t["cb"], paths, W, n).cpu().numpy()
    worst = 0.0
    for d in range(L):
        Wd = hip.zeros(n)
        md = hip.lsm_dates_moments(b.book, jt[:d + 1], np.array([0, d + 1]), paths, Wd, n).cpu().numpy()
        assert np.array_equal(_bits(md), _bits(mom[:d + 1])), d                        # a prefix of the chain: the same systems
        a = hip.resolve_atoms(b.book, [int(jt["num_atom"][d]), int(jt["x_atom"][d])], paths).cpu().numpy()
        z = (a[1] - jt["shift"][d]) * jt["scale"][d]
        ref, mag = R.moments_ref(z, a[0][None, :] * Wd.cpu().numpy()[None, :], K)
        bound = C_MOM * (2 * K + math.log2(n)) * R.EPS * mag
        err = np.abs(mom[d] - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (d, np.nonzero(err > bound)[0], mom[d], ref, err / np.maximum(bound, 1e-300))
    assert torch.equal(Wd, W)
    print("LSM-DATES moments: worst err / bound", worst)


# ---- controller level ---------------------------------------------------------------------------------------------------------------------
def _run(name, hip, flag, inject=True, **attrs):
    sc, g = cases.make_controller(name, hip, inject=inject)
    sc.date_batched_lsm = flag
    for k, v in attrs.items():
        setattr(sc, k, v)
    return sc, g, sc.run_simulation()


def _n_systems(sc, stateless_only=True):
    jobs, _ = sc._regression_plan()
    return sum(len(s) for _, p, s, _ in jobs if p.get_num_states() == 1 or not stateless_only)


def _same_results(ra, rb):
    assert ra.results == rb.results, (ra.results, rb.results)


@pytest.mark.parametrize("name", ["netting", "mixed_cva"])
def test_books_of_four_or_more_stateless_products_are_bitwise_identical(name, hip):
    off, _, r_off = _run(name, hip, False)
    on, _, r_on = _run(name, hip, True)
    assert off.lsm_routes["dates"] == 0 and off.lsm_routes["batched_steps"] > 0 and off.lsm_routes["per_product"] == 0
    assert on.lsm_routes == {"dates": _n_systems(on), "batched_steps": 0, "per_product": 0} and on.lsm_routes["dates"] > 0
    _same_results(r_on, r_off)
    for a, c in zip(on.regression_coeffs, off.regression_coeffs):
        assert torch.equal(a, c)
    for p, q in zip(on.products, off.products):
        assert torch.equal(torch.as_tensor(p.regression_coeffs), torch.as_tensor(q.regression_coeffs))
    assert np.array_equal(on.book.plan.coeffs, off.book.plan.coeffs)
    for key in ("paths", "cfs", "expo"):
        a, c = on.last_state.get(key), off.last_state.get(key)
        assert (a is None) == (c is None) and (a is None or torch.equal(a, c)), key


@pytest.mark.parametrize("name", ["irs_cva", "irs_cva_linspace", "zcb_cva"])
def test_per_product_books_meet_their_reference_fixtures(name, hip):
    """books of one product: the off route is mcx_lsm_run (another tiling), so the fixtures and their tolerances are the check"""
    from test_hip_parity import _check_against_golden
    on, g, res = _run(name, hip, True)
    assert on.lsm_routes == {"dates": _n_systems(on), "batched_steps": 0, "per_product": 0} and on.lsm_routes["dates"] > 0
    _check_against_golden(on, res, g, name + "[dates]")


def test_mixed_book_splits_between_the_two_routes(hip):
    from test_hip_parity import _check_against_golden
    on, g, res = _run("mixed_book_multi", hip, True)
    n_all, n_dates = _n_systems(on, stateless_only=False), _n_systems(on)
    assert 0 < n_dates < n_all and on.lsm_routes["dates"] == n_dates
    assert on.lsm_routes["batched_steps"] > 0 and on.lsm_routes["per_product"] == 0      # six exercise products: the batched route
    _check_against_golden(on, res, g, "mixed_book_multi[dates]")
    off, _, r_off = _run("mixed_book_multi", hip, False)
    _same_results(res, r_off)                                                            # (both groups bit-equal to the batched route)


def test_forward_mode_follows_the_flag(hip, monkeypatch):
    from test_oracle_golden import check_lsm_sensitivities
    calls = []
    inner = hip.lsm_dates_run
    monkeypatch.setattr(hip, "lsm_dates_run", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    on, g, res = _run("irs_cva_aad", hip, True)
    assert calls, "the base run of the differentiation did not take the date-batched route"
    check_lsm_sensitivities(on, g, res)


def test_singular_flag_takes_the_existing_fallback(hip, monkeypatch):
    off, _, r_off = _run("netting", hip, False)
    inner = hip.lsm_dates_run
    monkeypatch.setattr(hip, "lsm_dates_run", lambda *a, **k: (inner(*a, **k), 1)[1])
    on, _, r_on = _run("netting", hip, True)
    assert on.lsm_singular_retries == 1 and on.lsm_routes["dates"] == 0 and on.lsm_routes["batched_steps"] > 0
    # the fallback is the flag-off route with host solves (what that route does after a singular flag of its own): bit for bit
    host, _, r_host = _run("netting", hip, False, _lsm_host_solves=True)
    assert getattr(host, "lsm_singular_retries", 0) == 0
    _same_results(r_on, r_host)
    # and the host solver against the device solver of the plain flag-off run, under the fixture's tolerances
    from test_hip_parity import _check_against_golden
    _check_against_golden(on, r_on, cases.load_golden("netting"), "netting[fallback]")
    _check_against_golden(off, r_off, cases.load_golden("netting"), "netting[off]")
