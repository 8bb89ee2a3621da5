"""The interpreter kernel of the one-launch pass (kf_fused.hip) on books that mix straight-line and interpreted dates.

In a one-netting-set book kf_fused runs every date that has a straight-line FastDate record through kf_lean's `lean_date` and
every other date through the chunk interpreter `kf_on_date`.  Here every launch branch of `launch_kf` (injected draws or Philox,
one or several netting sets, with or without exercise products, NPF = 0 / 1 / 2 prefetch pieces) runs simulating
(main_plan="fused") and streaming a paths tensor (main_plan="semi"), on Black-Scholes and Vasicek + CIR++ (Euler) books, against
the CPU oracle on identical Philox counters or identical injected draws.  Before any number is compared, every test asks the
library (mcx_fused_describe, the host function the launch itself uses) which kernel, which template bounds and which date mix it
runs, and asserts the route it claims to test.  The last test checks that the module as a whole reached every launch branch,
every FastDate flag bit lean_date branches on and every date pattern listed in its docstring."""
import numpy as np
import pytest

import cases
from mcx import _abi
from mcx.plan import SimPlan

pytestmark = pytest.mark.gpu

MAXS = _abi.FUSED_MAX_STATEFUL
BIG = (1 << 19) + 333            # > 2048 tiles of 256 paths: grid-stride tiles (first_tile == false)
HUGE = 1_200_001                 # 4688 tiles on 1563 blocks: unequal tiles per block
# what the module has run, checked by test_module_coverage
SEEN = {"routes": set(), "flags": 0, "patterns": set(), "n_ns": set()}


# ---- books ------------------------------------------------------------------------------------------------------------------
def _euro(t, k, call, name):
    o = cases.EuropeanOption(cases.Equity(), t, k, cases.OptionType.CALL if call else cases.OptionType.PUT)
    o.name = name
    return o


def bs_book(n_bin=1, americans=(), n_ns=1, euler=False):
    """Black-Scholes, PV: plain European payoffs at 0.25 and 1.0 (straight-line dates), `n_bin` binary options at 0.5 (one
    interpreted date whose chunk grows with n_bin: the NPF bucket), optional American puts (exercise products, (dates, strike)
    each).  (No exposure metric: analytic Black-Scholes exposures are not fusable.)"""
    model = cases.BlackScholesModel(0, 100.0, 0.03, 0.25)
    P = [_euro(0.25, 95.0, True, "call_q"), _euro(1.0, 105.0, False, "put_1y")]
    for k in range(n_bin):
        b = cases.BinaryOption(0.5, 92.0 + 2.0 * k, 5.0 + k, cases.OptionType.CALL if k % 2 == 0 else cases.OptionType.PUT)
        b.name = f"binary_{k}"
        P.append(b)
    for j, (m, strike) in enumerate(americans):
        a = cases.AmericanOption(cases.Equity(), 1.0, m, strike, cases.OptionType.PUT)
        a.name = f"american_{j}"
        P.append(a)
    ns = [cases.NettingSet(name=f"ns{q}", products=P[q::n_ns]) for q in range(n_ns)]
    n_pre = 4096 if americans else 0
    return ns, model, cases.RiskMetrics([cases.PVMetric()]), n_pre, 3 if euler else 2, cases.E if euler else cases.A


HAZARDS = {0.5: 0.0064, 1.0: 0.0155, 2.0: 0.0097, 3.0: 0.0156, 5.0: 0.0228}


def irs_book(bond_opts=1, n_ns=1, epe=False, threshold=0.0, horizon=2.0):
    """Vasicek + CIR++ (Euler) payer swaps to 2.0 with CVA; European options on a coupon bond expiring at 1.0 (more than four
    exponential terms: an interpreted date between straight-line swap dates); exposure dates every quarter to `horizon` (past
    2.0: metric operations on dates without events)"""
    ir = cases.VasicekModel(0.0, 0.03, 0.05, 0.1, 0.01, asset_id="irs")
    cr = cases.CIRPPModel(0.0, "cp", HAZARDS, kappa=0.1, theta=0.01, volatility=0.02, y0=1e-4)
    model = cases.ModelConfig([ir, cr], inter_asset_correlation_matrix=np.array([0.5]))
    P = []
    for q in range(n_ns):
        s = cases.InterestRateSwap(0.0, 2.0, 1.0, 0.03 + 0.002 * q, 0.25, 0.25, cases.IRSType.PAYER, "irs")
        s.name = f"swap_{q}"
        P.append(s)
    for k in range(bond_opts):
        o = cases.EuropeanOption(cases.Bond(0.0, 3.0, 1.0, 0.5, True, 0.04, "irs"), 1.0, 0.98 + 0.01 * k, cases.OptionType.CALL, asset_id="irs")
        o.name = f"bond_call_{k}"
        P.append(o)
    ns = [cases.NettingSet(name=f"ns{q}", products=P[q::n_ns], counterparty_id="cp", threshold=threshold) for q in range(n_ns)]
    mets = [cases.CVAMetric("cp", 0.4)] + ([cases.EPEMetric()] if epe else [])
    return ns, model, cases.RiskMetrics(mets, exposure_timeline=np.arange(0.0, horizon + 1e-9, 0.25)), 4096, 2, cases.E


def berm_book(vol=0.01):
    """Vasicek + CIR++ (Euler), CVA: a Bermudan payer swaption on a 3-year swap (exercise values as value polynomials,
    state-indexed exposures).  With a zero CIR++ start (the test patches it in) every date is straight-line but the book runs
    kf_fused: the only way a state-indexed exposure reaches lean_date there (any second product adds an exposure event beside it)"""
    ir = cases.VasicekModel(0.0, 0.03, 0.05, 0.1, vol, asset_id="irs")
    cr = cases.CIRPPModel(0.0, "cp", HAZARDS, kappa=0.1, theta=0.01, volatility=0.02, y0=1e-4)
    model = cases.ModelConfig([ir, cr], inter_asset_correlation_matrix=np.array([0.5]))
    und = cases.InterestRateSwap(0.0, 3.0, 1.0, 0.03, 0.25, 0.25, cases.IRSType.PAYER, "irs")
    berm = cases.BermudanOption(und, [0.6, 1.2, 1.8, 2.4], 0.0, cases.OptionType.CALL, asset_id="irs")
    ns = [cases.NettingSet(name="berm_ns", products=[berm], counterparty_id="cp")]
    rm = cases.RiskMetrics([cases.CVAMetric("cp", 0.4)], exposure_timeline=np.arange(0.0, 3.0 + 1e-9, 0.25))
    return ns, model, rm, 4096, 2, cases.E


# ---- running and comparing --------------------------------------------------------------------------------------------------
def _controller(book, be, n, plan, materialize, inject, setup=None):
    ns, model, rm, n_pre, steps, scheme = book()
    sc = cases.SimulationController(ns, model, rm, n, n_pre, steps, scheme, backend=be)
    sc.materialize = materialize
    if plan is not None:
        sc.main_plan = plan
    if setup is not None:
        setup(sc)
    if inject:
        sp = SimPlan(sc.model, sc.simulation_timeline.numpy(), sc.simulation_scheme, sc.num_steps)
        rng = np.random.default_rng(20261016 + n)
        z = rng.standard_normal((sp.n_steps, sp.n_z, n))
        u = rng.uniform(size=(sp.n_steps, n)) if sp.n_uniform else None
        sc._inject["main"] = (be.from_numpy(z), be.from_numpy(u) if u is not None else None)
    return sc


_ORACLE = {}


def _oracle_run(key, book, n, inject, oracle, setup=None):
    """the oracle's materialised run of a (book, n, draws) case, shared by every HIP plan of the case"""
    if key not in _ORACLE:
        sc = _controller(book, oracle, n, None, True, inject, setup)
        res = sc.run_simulation()
        st = {k: (None if v is None else v.numpy().copy()) for k, v in sc.last_state.items() if k in ("paths", "cfs", "expo")}
        _ORACLE.clear()                    # one case at a time: the arrays of a 1.2 M-path case are large
        _ORACLE[key] = (res.results, st, sc)
    return _ORACLE[key]


def _patterns(valid):
    v = [int(x) for x in valid]
    pats = set()
    if 0 in v and 1 in v:
        pats.add("mixed")
    if any(v[t] == 1 and v[t + 1] == 0 for t in range(len(v) - 1)):
        pats.add("sl->int")
    if any(v[t] == 1 and v[t + 1] == 0 and 1 in v[t + 2:] for t in range(len(v) - 2)):
        pats.add("sl->int->sl")
    return pats


def _describe(hip, sc, inject, simulate, want):
    """the route of this controller's pass from the library, checked against `want` (kernel, nns, nst, npf: None = any)"""
    assert sc._fused is not None, getattr(hip, "not_fusable_reason", "not fusable")
    d = hip.fused_describe(sc._fused, inject, simulate)
    kernel, nns, nst, npf = want
    assert d["kernel"] == kernel, d
    if kernel == "fused":
        assert d["nns"] == nns and (nst is None or d["nst"] == nst) and (npf is None or d["kernel_npf"] == npf), d
    sl = d["valid"] == 1
    SEEN["flags"] |= int(np.bitwise_or.reduce(d["flags"][sl])) if sl.any() else 0
    pats = _patterns(d["valid"])
    if kernel == "fused":
        SEEN["routes"].add((bool(inject), d["n_ns"] == 1, d["n_stateful"] > 0, bool(simulate), d["nns"], d["nst"], d["kernel_npf"]))
        SEEN["n_ns"].add((d["nns"], d["n_ns"]))
        SEEN["patterns"].update((p, d["kernel_npf"]) for p in pats)
    return d


def _close_records(rh, ro, slack, tag):
    for ns_i in range(len(ro)):
        for m_i in range(len(ro[ns_i])):
            a, b = np.array(rh[ns_i][m_i], dtype=np.float64), np.array(ro[ns_i][m_i], dtype=np.float64)
            assert np.allclose(a[:, 0], b[:, 0], rtol=1e-8, atol=1e-10 + slack), (tag, ns_i, m_i, a[:, 0], b[:, 0])
            assert np.allclose(a[:, 1], b[:, 1], rtol=1e-5, atol=1e-11 + slack), (tag, ns_i, m_i, a[:, 1], b[:, 1])


def _close_entries(sh, so, exercise, tag):
    """paths, cashflows and exposures entry by entry; returns the record slack that paths whose exercise decision flipped at a
    near-tie explain (0 when none flipped)"""
    slack = 0.0
    for key in ("paths", "cfs", "expo"):
        a, b = sh[key], so[key]
        assert (a is None) == (b is None), (tag, key)
        if a is None:
            continue
        a = a.cpu().numpy()
        assert a.shape == b.shape, (tag, key, a.shape, b.shape)
        bad = ~np.isclose(a, b, rtol=1e-9, atol=1e-11)
        frac = bad.mean()
        assert frac <= (1e-4 if exercise and key != "paths" else 0.0), (tag, key, frac, np.abs(a - b).max())
        if bad.any():
            slack = max(slack, float(np.abs(a - b)[bad].max()) * bad.sum(axis=-1).max() / a.shape[-1])
    return slack


def _run_case(hip, oracle, key, book, n, plan, inject, want, exercise=False, setup=None):
    """one book on the HIP plan `plan` (materialised, then not) against the oracle; returns the route description"""
    rh_o, st_o, _ = _oracle_run(key, book, n, inject, oracle, setup)
    d = None
    slack = 0.0
    for materialize in (True, False):
        sc = _controller(book, hip, n, plan, materialize, inject, setup)
        res = sc.run_simulation()
        d = _describe(hip, sc, inject, plan == "fused", want)      # the route of the object this run launched, before any number
        tag = (key, plan, materialize)
        if materialize:
            for k in ("paths", "cfs", "expo"):
                if k == "paths" or st_o[k] is not None:
                    assert sc.last_state[k] is not None, (tag, k)
            slack = _close_entries(sc.last_state, st_o, exercise, tag)
        else:
            assert plan == "semi" or sc.last_state["paths"] is None, tag
        _close_records(res.results, rh_o, slack, tag)
    return d


# ---- launch branches --------------------------------------------------------------------------------------------------------
# id -> (book, paths, injected draws, one netting set, exercise products, object NPF (None: any), [plans])
ROUTES = {
    "bs-npf1": (lambda: bs_book(n_bin=1), 200, False, 1, 0),
    "bs-npf2": (lambda: bs_book(n_bin=6, euler=True), 70001, False, 1, 0),
    "bs-npf0": (lambda: bs_book(n_bin=12), HUGE, False, 1, 0),
    "bs-american-npf1": (lambda: bs_book(n_bin=1, americans=[(5, 100.0)]), 70001, False, 1, 1),
    "bs-american-npf2": (lambda: bs_book(n_bin=6, americans=[(5, 100.0)]), 200, False, 1, 1),
    "bs-american-npf0": (lambda: bs_book(n_bin=12, americans=[(5, 100.0)], euler=True), 70001, False, 1, 1),
    "bs-2ns": (lambda: bs_book(n_bin=2, n_ns=2), 70001, False, 2, 0),
    "bs-2ns-american": (lambda: bs_book(n_bin=2, n_ns=2, americans=[(5, 100.0)]), 200, False, 2, 1),
    "irs-4ns": (lambda: irs_book(bond_opts=1, n_ns=4), 70001, False, 4, 0),
    "irs-1ns": (lambda: irs_book(bond_opts=1), 70001, False, 1, 0),
    "bs-npf1-inject": (lambda: bs_book(n_bin=1), 70001, True, 1, 0),
    "bs-npf2-inject": (lambda: bs_book(n_bin=6), 200, True, 1, 0),
    "bs-npf0-inject": (lambda: bs_book(n_bin=12, euler=True), 70001, True, 1, 0),
    "irs-1ns-inject": (lambda: irs_book(bond_opts=1), 200, True, 1, 0),
    "bs-american-inject": (lambda: bs_book(n_bin=1, americans=[(5, 100.0)]), 70001, True, 1, 1),
    "bs-american-npf0-inject": (lambda: bs_book(n_bin=12, americans=[(5, 100.0)], euler=True), 200, True, 1, 1),
    "bs-2ns-inject": (lambda: bs_book(n_bin=2, n_ns=2, americans=[(5, 100.0)]), 70001, True, 2, 1),
    "irs-4ns-inject": (lambda: irs_book(bond_opts=1, n_ns=4), 200, True, 4, 0),
}
NPF_OF = {"npf0": 0, "npf1": 1, "npf2": 2}
PARAMS = [(k, p) for k, r in ROUTES.items() for p in (("fused",) if r[2] else ("fused", "semi"))]


def _want(key, n_ns, n_ex, inject, simulate):
    npf = next((v for s, v in NPF_OF.items() if s in key), None)
    if n_ns > 1:
        return ("fused", _abi.FUSED_MAX_NS, MAXS, 0)
    if n_ex == 0:
        return ("fused", 1, 0, npf)
    return ("fused", 1, MAXS, 0 if inject else npf)


@pytest.mark.parametrize("key,plan", PARAMS, ids=[f"{k}-{p}" for k, p in PARAMS])
def test_launch_branch_matches_oracle(key, plan, hip, oracle):
    book, n, inject, n_ns, n_ex = ROUTES[key]
    want = _want(key, n_ns, n_ex, inject, plan == "fused")
    d = _run_case(hip, oracle, key, book, n, plan, inject, want, exercise=n_ex > 0)
    assert d["n_ns"] == n_ns and (d["n_stateful"] > 0) == (n_ex > 0), d
    assert not d["lean"] and (d["valid"] == 0).any(), d         # some date runs the interpreter
    npf = next((v for s, v in NPF_OF.items() if s in key), None)
    if npf is not None:
        assert d["npf"] == npf, d
        lo, hi = {1: (1, 1024), 2: (1025, 2048), 0: (2049, 1 << 20)}[npf]
        assert lo <= d["max_chunk"] <= hi, d
    if n_ns == 1:
        assert (d["valid"] == 1).any(), d                       # and some date runs lean_date


# ---- date mixes in one netting set ------------------------------------------------------------------------------------------
def _two_americans(order):
    ams = [(5, 100.0), (4, 106.0)]
    return lambda: bs_book(n_bin=0, americans=ams if order == 0 else ams[::-1])


@pytest.mark.parametrize("inject", [False, True], ids=["philox", "inject"])
@pytest.mark.parametrize("order", [0, 1], ids=["five-dates-first", "four-dates-first"])
def test_two_exercise_products_hand_over_the_first_state(order, inject, hip, oracle):
    """two American puts on different exercise schedules: dates that carry only product 0 run lean_date on est[0], dates that
    carry product 1 run the interpreter, which reads and updates est[0] too (the shared dates 0 and 1.0)"""
    n = BIG if (order == 0 and not inject) else 70001
    plans = ("fused",) if inject else ("fused", "semi")
    for plan in plans:
        d = _run_case(hip, oracle, ("two_am", order, inject, n), _two_americans(order), n, plan, inject,
                      ("fused", 1, MAXS, 0 if inject else None), exercise=True)
        assert d["n_stateful"] == 2 and "sl->int->sl" in _patterns(d["valid"]), d
        assert (d["flags"][d["valid"] == 1] & _abi.FD_EXERCISE).all(), d     # every straight-line date is product 0's exercise


MIXES = {
    # constant numeraire, plain option payoffs beside exercise events
    "bs-american": (lambda: bs_book(n_bin=1, americans=[(5, 100.0)]), 70001, True),
    # merged CVA increment (no threshold, no profile), cashflows with exponential terms, one and two exposure rows
    "irs-cva": (lambda: irs_book(bond_opts=1), 200, False),
    # CVA with a threshold and EPE / ENE records (no merged increment), metric operations on dates without events
    "irs-cva-threshold-epe": (lambda: irs_book(bond_opts=1, epe=True, threshold=0.002, horizon=2.5), BIG, False),
}


@pytest.mark.parametrize("key", list(MIXES))
@pytest.mark.parametrize("plan", ["fused", "semi"])
def test_mixed_dates_match_oracle(key, plan, hip, oracle):
    book, n, exercise = MIXES[key]
    d = _run_case(hip, oracle, key, book, n, plan, False, ("fused", 1, None, None), exercise=exercise)
    assert {"mixed", "sl->int->sl"} <= _patterns(d["valid"]), d


def test_value_polynomial_fallback_inside_the_interpreter(hip, oracle, monkeypatch):
    """a volatile short rate and value polynomials verified on a range narrower than the pre-simulation's: waves that hold a
    path outside [ex_p_lo, ex_p_hi] run lean_date's term loop inside kf_fused, the others the polynomial; the exposures read
    the coefficient row of each lane's exercise state"""
    from mcx.models.cirpp import CIRPPModel
    monkeypatch.setattr(CIRPPModel, "_initial_state", lambda self: [0.0, 0.0])

    def narrow(sc):
        sc.collapse_pad = -0.25
    book = lambda: berm_book(vol=0.03)
    for plan in ("fused", "semi"):
        d = _run_case(hip, oracle, "berm", book, 70001, plan, False, ("fused", 1, MAXS, None), exercise=True, setup=narrow)
        assert not d["lean"] and (d["valid"] == 1).all() and d["max_chunk"] == 0, d
        assert (d["flags"] & _abi.FD_EX_VPOLY).any() and (d["flags"] & _abi.FD_STATE_EXPO).any(), d
    # the paths of that run leave the verified range on some exercise date (read back from the library)
    import ctypes as C
    sc = _controller(book, hip, 70001, "fused", True, False, narrow)
    sc.run_simulation()
    paths = sc.last_state["paths"].cpu().numpy()
    ev = sc.book_plan.events
    outside = inside = 0
    for q in range(len(ev)):
        nb, lo, hi = C.c_int32(), C.c_double(), C.c_double()
        if hip.lib.mcx_book_value_poly_info(sc.book.ptr, C.c_int32(q), C.byref(nb), C.byref(lo), C.byref(hi)) != 1:
            continue
        x = paths[int(ev["t_idx"][q]), 0]                  # the short rate (state column 0), the polynomial's variable
        out = (x < lo.value) | (x > hi.value)
        outside += int(out.sum())
        inside += int((~out).sum())
    assert outside > 0 and inside > 0, (outside, inside)


def test_module_coverage():
    """every launch branch, FastDate flag bit and date pattern the module claims (the union over the tests above)"""
    need_routes = set()
    for sim in (True, False):
        for npf in (0, 1, 2):
            need_routes.add((False, True, False, sim, 1, 0, npf))
            need_routes.add((False, True, True, sim, 1, MAXS, npf))
        need_routes.add((False, False, False, sim, _abi.FUSED_MAX_NS, MAXS, 0))
        need_routes.add((False, False, True, sim, _abi.FUSED_MAX_NS, MAXS, 0))
    for npf in (0, 1, 2):
        need_routes.add((True, True, False, True, 1, 0, npf))
    need_routes.add((True, True, True, True, 1, MAXS, 0))
    need_routes.add((True, False, False, True, _abi.FUSED_MAX_NS, MAXS, 0))
    need_routes.add((True, False, True, True, _abi.FUSED_MAX_NS, MAXS, 0))
    assert need_routes <= SEEN["routes"], sorted(need_routes - SEEN["routes"])
    assert {(_abi.FUSED_MAX_NS, 2), (_abi.FUSED_MAX_NS, 4)} <= SEEN["n_ns"], SEEN["n_ns"]
    flags = (_abi.FD_CASH | _abi.FD_EXPO | _abi.FD_CVA | _abi.FD_PROFILE | _abi.FD_CONST_NUM | _abi.FD_METRIC | _abi.FD_MERGED |
             _abi.FD_EXERCISE | _abi.FD_STATE_EXPO | _abi.FD_OPTION | _abi.FD_EX_VPOLY)
    assert SEEN["flags"] & flags == flags, hex(flags & ~SEEN["flags"])
    # an interpreted date right after a straight-line one, its chunk from the prefetch issued in the straight-line branch
    assert {("sl->int", 1), ("sl->int", 2), ("sl->int->sl", 0)} <= SEEN["patterns"], SEEN["patterns"]
