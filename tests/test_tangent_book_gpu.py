"""What the forward-mode book pass (csrc/kt_book.hip) keeps on the handle and in the book instead of allocating per call:

  1. the id tables of a book are uploaded once and cached in the book: two books on one handle, calls interleaved, one destroyed on the
     way, give the bytes of the same calls on a fresh book alone;
  2. a host table above a quarter of the staging ring goes through a scratch buffer of the handle: the dates two simulations share
     come out equal whichever branch the table took;
  3. tables staged through the ring survive its half-ring turnovers: many calls, one result;
  4. one predicate decides which events have a tangent form: the three callers refuse the same event, each in its own words."""
import gc

import numpy as np
import pytest
import torch

import cases
from mcx import _abi
from mcx._native import McxError
from mcx.plan import SimPlan

pytestmark = pytest.mark.gpu
NP = _abi.TANGENT_NP
RING = 4 << 20                                                                # the handle's staging ring (csrc/mcx_api.hip)


def _staged(n_bytes):
    return (n_bytes + 255) // 256 * 256


# ---- 1. two books, one handle ------------------------------------------------------------------------------------------------------
def _second_book():
    """three products on mixed_cva's models, in another order and with other schedules: other event counts, another term -> atom map"""
    _, model, _ = cases.mixed_cva()
    s = cases.InterestRateSwap(0.0, 1.5, 10.0, 0.03, 0.5, 0.25, cases.IRSType.RECEIVER, "rates"); s.name = "swap1"
    o = cases.EuropeanOption(cases.Equity("equity"), 1.5, 100.0, cases.OptionType.PUT, asset_id="equity"); o.name = "put0"
    b = cases.Bond(0.0, 1.0, 1.0, 0.25, True, 0.03, "rates"); b.name = "bond1"
    ns = [cases.NettingSet(name="second", products=[s, o, b], counterparty_id="cp")]
    return ns, model, cases.RiskMetrics([cases.CVAMetric("cp", 0.4), cases.EPEMetric()], exposure_timeline=np.linspace(0.0, 1.5, 7))


def _book_inputs(build, hip, n, seed):
    """a book plan with everything tangent_lsm, tangent_eval and tangent_cva need at n paths; the controller and its book are gone"""
    from mcx.aad import stateless_lsm_jobs
    ns, model, rm = build()
    sc = cases.SimulationController(ns, model, rm, n, n, 2, cases.E, backend=hip)
    sc.materialize = True
    sc.run_simulation()
    rng = np.random.default_rng(seed)
    plan = sc._sim.plan
    paths, dpaths = hip.tangent_paths(sc._sim, rng.normal(0.0, 0.05, (plan.n_slots, _abi.SLOT_NPARAM, NP)), rng.normal(0.0, 0.05, (plan.n_state, NP)),
                                      rng.normal(0.0, 0.05, (plan.n_steps, plan.n_slots, _abi.AUX, NP)), 42, 0, n)
    bp = sc.book_plan
    h_datoms = rng.normal(0.0, 0.3, (len(bp.atoms), 5, NP))
    h_datoms[:, 3:] *= 0.1
    lsm_plan, _ = sc._regression_plan()
    x_ids = sorted({x for _, _, _, atoms in lsm_plan for _, x in atoms})
    stats = hip.lsm_stats(sc.book, x_ids, paths)
    table, _ = stateless_lsm_jobs(lsm_plan, {x: (stats[i, 0], stats[i, 1]) for i, x in enumerate(x_ids)}, sc._expo_coeff_base, bp.n_basis)
    coeffs = rng.normal(0.0, 0.5, len(bp.coeffs))
    surv, cond = sc._cva_atoms[0]
    inp = dict(plan=bp, table=table, datoms=hip.from_numpy(h_datoms), paths=paths, dpaths=dpaths, coeffs=hip.from_numpy(coeffs),
               dcoeffs=hip.from_numpy(rng.normal(0.0, 0.1, (len(coeffs), NP))), rows=sc.metric_exposure_indices.numpy().astype(np.int32),
               surv=np.array(surv, dtype=np.int32), cond=np.array(cond, dtype=np.int32))
    del sc
    gc.collect()
    return inp


def _lsm(hip, book, x, j):
    q = x["table"][j]
    return hip.tangent_lsm(book, int(q["product"]), int(q["first_event"]), int(q["num_atom"]), int(q["x_atom"]), float(q["shift"]),
                           float(q["scale"]), x["datoms"], x["paths"], x["dpaths"]).tobytes()


def _eval(hip, book, x):
    cfs, expo = hip.tangent_eval(book, x["datoms"], x["coeffs"], x["dcoeffs"], x["paths"], x["dpaths"])
    return cfs.cpu().numpy().tobytes() + expo.cpu().numpy().tobytes(), expo


def _cva(hip, book, x, expo):
    return hip.tangent_cva(book, x["datoms"], x["rows"], x["surv"], x["cond"], 0.0, 0.4, expo, 0, x["paths"], x["dpaths"]).cpu().numpy().tobytes()


def test_two_books_on_one_handle_keep_their_own_id_tables(hip):
    n = 257
    A, B = _book_inputs(cases.mixed_cva, hip, n, 1), _book_inputs(_second_book, hip, n, 2)
    assert len(A["plan"].events) != len(B["plan"].events) and len(A["plan"].terms) != len(B["plan"].terms)
    assert len(A["plan"].products) == 4 and len(B["plan"].products) == 3 and len(A["table"]) >= 2 and len(B["table"]) >= 2
    ref = {}
    for tag, x in (("A", A), ("B", B)):                                       # every call on a fresh book, no other book alive
        for j in (0, 1):
            book = hip.book_create(x["plan"])
            ref[tag, "lsm", j] = _lsm(hip, book, x, j)
            del book
        book = hip.book_create(x["plan"])
        ref[tag, "eval"], expo = _eval(hip, book, x)
        del book
        book = hip.book_create(x["plan"])
        ref[tag, "cva"] = _cva(hip, book, x, expo)
        del book, expo
    assert ref["A", "lsm", 0] != ref["A", "lsm", 1] and ref["A", "cva"] != ref["B", "cva"]
    a, b = hip.book_create(A["plan"]), hip.book_create(B["plan"])
    assert _lsm(hip, a, A, 0) == ref["A", "lsm", 0]
    assert _lsm(hip, b, B, 0) == ref["B", "lsm", 0]
    got, expo_a = _eval(hip, a, A)
    assert got == ref["A", "eval"]
    got, expo_b = _eval(hip, b, B)
    assert got == ref["B", "eval"]
    assert _cva(hip, a, A, expo_a) == ref["A", "cva"]
    assert _lsm(hip, b, B, 1) == ref["B", "lsm", 1]
    assert _cva(hip, b, B, expo_b) == ref["B", "cva"]
    assert _lsm(hip, a, A, 1) == ref["A", "lsm", 1]
    del a                                                                     # mcx_book_destroy: the first book's tables go, the second's stay
    gc.collect()
    assert _lsm(hip, b, B, 0) == ref["B", "lsm", 0]
    got, expo_b = _eval(hip, b, B)
    assert got == ref["B", "eval"]
    assert _cva(hip, b, B, expo_b) == ref["B", "cva"]


# ---- 2. a table too large for the ring -----------------------------------------------------------------------------------------------
def _four_slot_model():
    eq = cases.BlackScholesModel(0.0, 100.0, 0.03, 0.22, asset_id="equity")
    e2 = cases.BlackScholesModel(0.0, 50.0, 0.02, 0.3, asset_id="equity2")
    ra = cases.VasicekModel(0.0, 0.03, 0.03, 1.0, 0.01, asset_id="rates")
    cr = cases.CIRPPModel(0.0, "cp", cases.HAZARDS, kappa=0.10, theta=0.01, volatility=0.02, y0=1e-4)
    return cases.ModelConfig([eq, e2, ra, cr], inter_asset_correlation_matrix=[np.array([0.1])] * 6)


def test_a_table_above_a_quarter_of_the_ring_takes_the_scratch_buffer(hip):
    """11 intervals of 100 sub-steps against the first 2 of them: the same sub-step table as far as the short one goes"""
    long, short = (SimPlan(_four_slot_model(), 0.125 * np.arange(k), cases.E, 100) for k in (12, 3))
    assert (long.n_slots, long.n_steps, short.n_steps) == (4, 1100, 200)
    assert np.array_equal(long.steps[:200], short.steps) and np.array_equal(long.aux[:200], short.aux)
    rng = np.random.default_rng(5)
    dslot, dinit = rng.normal(0.0, 0.05, (4, _abi.SLOT_NPARAM, NP)), rng.normal(0.0, 0.05, (long.n_state, NP))
    daux = rng.normal(0.0, 0.05, (1100, 4, _abi.AUX, NP))
    assert daux[0, 0].nbytes == 256 and daux.nbytes > RING // 4 >= daux[:200].nbytes        # scratch buffer; ring
    p_long, dp_long = hip.tangent_paths(hip.sim_create(long), dslot, dinit, daux, 7, 0, 64)
    p_short, dp_short = hip.tangent_paths(hip.sim_create(short), dslot, dinit, daux[:200], 7, 0, 64)
    assert p_short.shape == (3, long.n_state, 64) and dp_long.shape == (NP, 12, long.n_state, 64)
    assert p_long[:3].cpu().numpy().tobytes() == p_short.cpu().numpy().tobytes()
    assert dp_long[:, :3].contiguous().cpu().numpy().tobytes() == dp_short.cpu().numpy().tobytes()
    assert float(dp_short[:, 2].abs().max()) > 0.0 and not bool(torch.isnan(dp_long).any())


# ---- 3. the ring turns over ----------------------------------------------------------------------------------------------------------
def test_tangent_cva_tables_survive_the_ring_turning_over(hip):
    n, n_dates = 64, 512                                                      # MCX_MAX_METRIC_DATES
    x = _book_inputs(cases.mixed_cva, hip, n, 3)
    book = hip.book_create(x["plan"])
    _, expo = _eval(hip, book, x)
    n_rows = expo.shape[2]
    rows = (np.arange(n_dates) % n_rows).astype(np.int32)
    delayed = np.where(np.arange(n_dates) % 3 == 0, -1, (np.arange(n_dates) + 1) % n_rows).astype(np.int32)
    surv, cond = np.resize(x["surv"], n_dates - 1), np.resize(x["cond"], n_dates - 1)
    per_call = _staged(rows.nbytes) + _staged(delayed.nbytes) + _staged(surv.nbytes) + _staged(cond.nbytes)
    assert per_call == 4 * 2048
    calls = 2 * -(-(RING // 2) // per_call) + 1                               # two half-ring boundaries wherever the cursor starts
    first = None
    for _ in range(calls):
        out = hip.tangent_cva(book, x["datoms"], rows, surv, cond, 0.01, 0.4, expo, 0, x["paths"], x["dpaths"], delayed, True)
        if first is None:
            first = out
            assert float(first[1:].abs().max()) > 0.0 and not bool(torch.isnan(first).any())
        else:
            assert torch.equal(out.view(torch.int64), first.view(torch.int64))


# ---- 4. refusals: one predicate, three callers -----------------------------------------------------------------------------------------
def _binary_book(hip):
    model = cases.BlackScholesModel(0.0, 100.0, 0.03, 0.2, asset_id="asset")
    call = cases.EuropeanOption(cases.Equity("asset"), 1.0, 100.0, cases.OptionType.CALL, asset_id="asset"); call.name = "call"
    binary = cases.BinaryOption(1.0, 100.0, 10.0, cases.OptionType.CALL, asset_id="asset")
    sc = cases.SimulationController([cases.NettingSet(name="bin", products=[call, binary])], model, cases.RiskMetrics([cases.PVMetric()]),
                                    256, 0, 2, cases.E, backend=hip)
    sc.materialize = True
    sc.run_simulation()
    return sc


@pytest.fixture(scope="module")
def refusal_books(hip):
    """(book, product, {caller: event index or None}) per offending event, and the tensors every call takes"""
    sc = _binary_book(hip)
    ev, pr = sc.book_plan.events, sc.book_plan.products
    exotic = lambda q: ev["kind"][q] == _abi.EV_OPTION and ev["aux"][q][0] != 0.0
    assert all(not exotic(q) for q in range(pr["ev_begin"][0], pr["ev_end"][0])) and exotic(pr["cf_begin"][1]) and exotic(pr["ev_begin"][1])
    out = {"binary": (sc.book, 1, {"cf": int(pr["cf_begin"][1]), "ev": int(pr["ev_begin"][1])})}
    # an option over per-term denominators (the compiler emits none: the plain call's terms get one by hand)
    sd = _binary_book(hip)
    plan = sd.book_plan
    for q in (int(pr["cf_begin"][0]), int(pr["ev_begin"][0])):
        assert plan.events["kind"][q] == _abi.EV_OPTION and plan.events["aux"][q][0] == 0.0
        plan.terms["den"][plan.events["term_begin"][q]:plan.events["term_end"][q]] = 0
    out["term_den"] = (hip.book_create(plan), 0, {"cf": None, "ev": None})
    paths = sc.last_state["paths"].contiguous()
    n = paths.shape[2]
    t = dict(datoms=hip.zeros(len(plan.atoms), 5, NP), paths=paths, dpaths=hip.zeros(NP, *paths.shape), W=hip.zeros(1, n), dW=hip.zeros(NP, 1, n),
             coeffs=hip.zeros(len(plan.coeffs)), dcoeffs=hip.zeros(len(plan.coeffs), NP))
    return out, t, (sc, sd)


@pytest.mark.parametrize("caller", ["mcx_tangent_lsm", "mcx_tangent_lsm_step", "mcx_tangent_eval"])
@pytest.mark.parametrize("event", ["binary", "term_den"])
def test_the_three_callers_refuse_the_same_event(event, caller, refusal_books, hip):
    books, t, _ = refusal_books
    book, product, index = books[event]
    pr = book.plan.products
    with pytest.raises(McxError) as e:
        if caller == "mcx_tangent_lsm":
            hip.tangent_lsm(book, product, 0, 0, 0, 0.0, 1.0, t["datoms"], t["paths"], t["dpaths"])
        elif caller == "mcx_tangent_lsm_step":
            hip.tangent_lsm_step(book, product, 0, int(pr["cf_end"][product] - pr["cf_begin"][product]), 0, 0, 0.0, 1.0, t["datoms"], t["paths"],
                                 t["dpaths"], t["W"], t["dW"])
        else:
            hip.tangent_eval(book, t["datoms"], t["coeffs"], t["dcoeffs"], t["paths"], t["dpaths"])
    msg = str(e.value)
    assert e.value.code == _abi.E_NOT_FUSABLE and caller + ":" in msg, msg
    if event == "binary":
        q = index["ev" if caller == "mcx_tangent_eval" else "cf"]
        assert f"event {q} (kind {_abi.EV_OPTION}" in msg and "has no tangent form" in msg, msg
        assert ("mode 3" in msg) == (caller != "mcx_tangent_eval"), msg       # the moment entry points name the option mode
    else:
        assert "option over per-term denominators" in msg, msg
