"""Every route of the step maps on the GPU, per path-step, against the long-double reference of step_reference.py.

One harness (step_reference.check_paths): every transition between stored dates is advanced in the reference from the kernel's
OWN stored state and the next stored state must lie within u * sens (u = 2^-50: what the kernels document per operation, sens
derived per entry by perturbing every rounded operation of the reference).  Draws are exact inputs: the injected tensors, or
rng_draws -> box_muller with the route's table size (10 bits for Vasicek + CIR++ on the one-launch kernel, 7 elsewhere; the QE
uniform is the first uniform of draw (n_z + 1) / 2).  Every route is asserted by name before a number is compared:
mcx_sim_describe for K1, mcx_fused_describe for the fused kernels.

Nothing is left out except: hard QE path-steps whose indicator margin lies inside its own bound AND whose two branches differ
(cap: none at these sizes; one that appears must match the other branch), and smoothed QE entries that are ill-conditioned
(bound > 1e-6 |value| or psi + eps changes sign inside its bound; cap 1e-3 of the finite path-steps per parameter set).
Measured on the MI355X: no near-branch path-step and no ill-conditioned entry, for any set on any route (smoothed sets 1, 7, 14, 21:
0 of 15650, 13485, 14352 and 47076 finite path-steps on the injected route); the worst ratios per route and step map are in
DESIGN §5 (0.12 for the fma-only maps, 0.29 - 0.54 CIR++, 0.43 - 0.65 QE).  On the edge block of the injected route the relative
criterion is not applied (those states cancel v' to nothing on purpose): they are checked like every other entry."""
import numpy as np
import pytest

import cases
import step_cases as sc
import step_reference as sr

pytestmark = pytest.mark.gpu


def _check(run, tag, n_edge=0):
    rep = sr.check_paths(run.tb, run.paths, run.draws, sr.U_KERNEL, n_edge=n_edge, explain=True)
    print("STEP-RATIO", tag, rep)
    rep.assert_ok(tag)
    assert rep.near_branch == 0, (tag, str(rep))
    assert rep.ill_conditioned <= 1e-3 * rep.finite_path_steps, (tag, str(rep))
    return rep


def _signature_of_case(name):
    kind, scheme = name.split("-")[0], name.split("-")[1]
    table = {("bs", "analytical"): "BS_A", ("bs", "euler"): "BS_E", ("vasicek", "analytical"): "VAS_A", ("vasicek", "euler"): "VAS_E",
             ("heston", "euler"): "HESTON_E", ("bs_vas_cirdet", "euler"): "BS_VAS_CIRDET_E"}
    return table.get((kind, scheme), "GENERIC")


# ---- route 1: K1, injected draws, per-path start states, edge states ---------------------------------------------------------------
@pytest.mark.parametrize("case", sc.INJECTED + sc.INJECTED_SPECIAL, ids=lambda c: c[0])
def test_k1_injected(case, hip):
    run = sc.run_injected(hip, sc.build_model(case), case[2], case[3], sc.N, case[4], edges=True)
    assert hip.sim_describe(run.sim)["signature"] == _signature_of_case(case[0]), case[0]
    _check(run, ("k1-injected", case[0]), run.n_edge)


QE_ALL = [(c, n, False) for v in sc.QE_HARD.values() for c, n in v] + [(sc.QE_CAP, 1, False)] + [(c, n, True) for c, n in sc.QE_SMOOTH]
QE_IDS = [f"{'smooth' if s else 'hard'}-{c}-{n}" for c, n, s in QE_ALL]


@pytest.mark.parametrize("case,nsub,smooth", QE_ALL, ids=QE_IDS)
def test_k1_injected_qe(case, nsub, smooth, hip):
    run = sc.run_injected(hip, sc.heston_qe(case, smooth), sc.Q, nsub, sc.N, 300 + case, edges=True)
    assert hip.sim_describe(run.sim)["signature"] == "HESTON_QE"
    rep = _check(run, ("k1-injected-qe", case, nsub, smooth), run.n_edge)
    assert bool(rep.nan_entries) == smooth


def test_k1_injected_floor_count_and_small_launch(hip):
    """CIR++ from y in {0, 1e-12, 1e-9, 0.05, -1e-4} with z = -8.5: the entries the floor catches are counted against the
    reference's (check_paths fails on any difference) and there are some; and one run of 63 paths"""
    case = next(c for c in sc.INJECTED_SPECIAL if c[0] == "cirpp-euler-floor")
    run = sc.run_injected(hip, sc.build_model(case), case[2], 1, sc.N, case[4], edges=True)
    rep = _check(run, "floor", run.n_edge)
    in_edge_block = int((run.paths[1, 0, :run.n_edge] == 1e-12).sum())
    print("STEP-RATIO floored in the edge block", in_edge_block, "of", run.n_edge, "; in the run", rep.floored)
    assert in_edge_block >= run.n_edge // 30 and rep.floored > in_edge_block, str(rep)       # (y = 0.05 with z = -8.5: every 30th edge path)
    small = sc.run_injected(hip, sc.build_model(case), case[2], 3, 63, case[4], edges=True)
    _check(small, "63 paths")
    # with injected draws the counter (path offset, sub-step, draw) is not read: a launch from path 2^33 + 12345 gives the same bits
    high = sc.run_injected(hip, sc.build_model(case), case[2], 1, sc.N, case[4], edges=True, path_offset=sc.OFFSET_BIG)
    assert np.array_equal(high.paths, run.paths)


# ---- routes 2 and 3: K1, Philox, specialised signatures and run-time dispatch -----------------------------------------------------
@pytest.mark.parametrize("case", sc.PHILOX, ids=lambda c: c[0])
def test_k1_philox(case, hip):
    run = sc.run_philox(hip, sc.build_model(case), case[2], case[3], sc.N)
    assert hip.sim_describe(run.sim)["signature"] == case[5], case[0]
    _check(run, ("k1-philox", case[5], case[0]))


@pytest.mark.parametrize("case,nsub,smooth", [q for q in QE_ALL if q[0] != sc.QE_CAP], ids=[i for i, q in zip(QE_IDS, QE_ALL) if q[0] != sc.QE_CAP])
def test_k1_philox_qe(case, nsub, smooth, hip):
    run = sc.run_philox(hip, sc.heston_qe(case, smooth), sc.Q, nsub, sc.N, path_offset=1000003 * case)
    assert hip.sim_describe(run.sim)["signature"] == "HESTON_QE"
    _check(run, ("k1-philox-qe", case, nsub, smooth))


@pytest.mark.parametrize("name", ["vas_cir+0.95-euler-0", "multi_cir-euler-0"], ids=["specialised", "generic"])
def test_k1_philox_high_path_offset_and_small_launch(name, hip):
    """paths from 2^33 + 12345 (the high counter word is not zero), and 63 paths"""
    case = next(c for c in sc.PHILOX if c[0] == name)
    for n, off in ((sc.N, sc.OFFSET_BIG), (63, 0)):
        run = sc.run_philox(hip, sc.build_model(case), case[2], 3, n, path_offset=off)
        assert hip.sim_describe(run.sim)["signature"] == case[5]
        _check(run, ("k1-philox", name, n, off))
    low = sc.run_philox(hip, sc.build_model(case), case[2], 3, 64, path_offset=12345)
    assert not np.array_equal(low.paths[1:, :, :63], sc.run_philox(hip, sc.build_model(case), case[2], 3, 64, path_offset=sc.OFFSET_BIG).paths[1:, :, :63])


# ---- routes 4 and 5: the one-launch kernel and the interpreter, simulating, one sub-step per date ------------------------------------
def _book(kind, rng):
    from mcx.products.bond import Bond
    if kind in ("BS_A", "BS_E"):
        # (a Black-Scholes exposure is analytic and evaluated by the book kernel, which makes a book unfusable: PV alone, one call
        #  per grid date; the timeline then starts at GRID[1] and the first transition starts from the model's own state)
        model, prods = sc.bs(rng), []
        for k, t in enumerate(sc.GRID[1:]):
            prods.append(cases.EuropeanOption(cases.Equity(), float(t), float(model._pf(0)), cases.OptionType.CALL))
            prods[-1].name = f"call{k}"
        return [cases.NettingSet(name="opts", products=prods)], model, cases.RiskMetrics([cases.PVMetric()])
    if kind in ("HESTON_E", "HESTON_QE", "HESTON_QE_SMOOTH"):
        # PV alone, one call per grid date, as for Black-Scholes; the QE sets are mixed sets of the sweep (9 hard, 7 smoothed)
        model = sc.heston_euler(rng) if kind == "HESTON_E" else sc.heston_qe(7 if kind.endswith("SMOOTH") else 9, kind.endswith("SMOOTH"))
        prods = []
        for k, t in enumerate(sc.GRID[1:]):
            prods.append(cases.EuropeanOption(cases.Equity(), float(t), float(model._pf(0)), cases.OptionType.CALL))
            prods[-1].name = f"call{k}"
        return [cases.NettingSet(name="opts", products=prods)], model, cases.RiskMetrics([cases.PVMetric()])
    if kind == "HW_A" or kind == "HW_E":
        model = sc.hw(rng)
        prod = Bond(0.0, float(sc.GRID[-1]), 1.0, float(sc.GRID[-1]), True, 0.0)
        return [cases.NettingSet(name="bond", products=[prod])], model, cases.RiskMetrics([cases.PVMetric(), cases.EPEMetric()], exposure_timeline=sc.GRID)
    if kind == "BS_VAS_CIRDET_E":
        model = sc.bs_vas_cirdet(rng)
        prod = Bond(0.0, float(sc.GRID[-1]), 1.0, float(sc.GRID[-1]), True, 0.0, "rates")
        return [cases.NettingSet(name="bond", products=[prod], counterparty_id="cp")], model, cases.RiskMetrics([cases.CVAMetric("cp", 0.4)], exposure_timeline=sc.GRID)
    if kind in ("VAS_E", "VAS_A"):
        model = sc.vas(rng, "ir")
        prod = Bond(0.0, float(sc.GRID[-1]), 1.0, float(sc.GRID[-1]), True, 0.0, "ir")
        return [cases.NettingSet(name="bond", products=[prod])], model, cases.RiskMetrics([cases.PVMetric(), cases.EPEMetric()], exposure_timeline=sc.GRID)
    model = sc.vas_cir(rng, 0.95 if rng.integers(0, 2) else -0.95)
    prod = Bond(0.0, float(sc.GRID[-1]), 1.0, float(sc.GRID[-1]), True, 0.0, "ir")
    return [cases.NettingSet(name="bond", products=[prod], counterparty_id="cp")], model, cases.RiskMetrics([cases.CVAMetric("cp", 0.4)], exposure_timeline=sc.GRID)


def _fused_controller(kind, hip, seed):
    ns, model, rm = _book(kind, np.random.default_rng(seed))
    scheme = sc.A if kind.endswith("_A") else sc.Q if "_QE" in kind else sc.E
    ctl = cases.SimulationController(ns, model, rm, sc.N, 1024, 1, scheme, backend=hip)
    ctl.main_plan, ctl.materialize = "fused", True
    ctl.prepare()
    assert ctl._fused is not None, hip.not_fusable_reason
    return ctl


def _fused_runs(hip, ctl, kernel, bits, tag):
    """Philox (n = 4097 from path 0 and from 2^33 + 12345, n = 63) and injected draws through mcx_fused_run with a paths tensor"""
    plan, f, seed = ctl.sim_plan, ctl._fused, ctl._main_engine.seed
    for inject in (False, True):
        d = hip.fused_describe(f, inject, True)
        assert d["kernel"] == kernel, (tag, inject, d)
        assert kernel == "fused" or (d["lean"] and (d["valid"] == 1).all()), (tag, d)
    assert np.array_equal(plan.timeline, sc.GRID[1 - plan.n_initial_store:]) and plan.n_steps == len(sc.GRID) - 1
    for n, off in ((sc.N, 0), (sc.N, sc.OFFSET_BIG), (63, 7)):
        paths = hip.empty(plan.n_dates, plan.n_state, n)
        hip.fused_run(f, seed, off, n, paths=paths)
        run = sc.Run(plan, paths.cpu().numpy(), sc.philox_draws(hip, plan, seed, off, n, bits))
        _check(run, (tag, "philox", n, off))
    rng = np.random.default_rng(11)
    z = rng.standard_normal((plan.n_steps, plan.n_z, sc.N))
    u = rng.random((plan.n_steps, sc.N)) if plan.n_uniform else None
    paths = hip.empty(plan.n_dates, plan.n_state, sc.N)
    hip.fused_run(f, seed, 0, sc.N, paths=paths, inject_z=hip.from_numpy(z), inject_u=hip.from_numpy(u) if u is not None else None)
    _check(sc.Run(plan, paths.cpu().numpy(), lambda k: (z[k], u[k] if u is not None else None)), (tag, "injected"))


# every signature the one-launch kernel accepts among those of the K1 routes (mcx_launch_kf_lean dispatches through
# mcx_dispatch_signature<4>: the eight named signatures and the run-time dispatch up to four slots; mcx_fused_create refuses only
# the Schwartz two-factor model and a CIR++ start at zero), each on a book whose every date is straight-line.  CIR++ alone cannot
# be booked: a credit model has no numeraire, so no product compiles on it.
ONE_LAUNCH = [("BS_A", 1, "BS_A"), ("BS_A", 2, "BS_A"), ("BS_E", 3, "BS_E"), ("BS_E", 4, "BS_E"), ("VAS_CIR_E", 5, "VAS_CIR_E"),
              ("VAS_CIR_E", 6, "VAS_CIR_E"), ("VAS_E", 7, "VAS_E"), ("VAS_A", 9, "VAS_A"), ("HESTON_E", 10, "HESTON_E"),
              ("HESTON_QE", 11, "HESTON_QE"), ("HESTON_QE_SMOOTH", 12, "HESTON_QE"), ("BS_VAS_CIRDET_E", 13, "BS_VAS_CIRDET_E"),
              ("HW_A", 14, "GENERIC"), ("HW_E", 15, "GENERIC")]


@pytest.mark.parametrize("kind,seed,signature", ONE_LAUNCH, ids=[f"{k}-{s}" for k, s, _ in ONE_LAUNCH])
def test_one_launch_kernel(kind, seed, signature, hip):
    ctl = _fused_controller(kind, hip, seed)
    assert hip.sim_describe(ctl._sim)["signature"] == signature
    _fused_runs(hip, ctl, "lean", 10 if kind == "VAS_CIR_E" else 7, ("one-launch", kind, seed))


def test_schwartz_two_factor_has_no_one_launch_kernel(hip):
    """the only model mcx_fused_create refuses: its spot is a derived state column"""
    ns, model, rm = cases.s2f_european()
    ctl = cases.SimulationController(ns, model, rm, sc.N, 0, 1, sc.E, backend=hip)
    ctl.main_plan = "fused"
    ctl.prepare()
    assert ctl._fused is None and "Schwartz two-factor" in hip.not_fusable_reason, hip.not_fusable_reason


def test_interpreter_with_a_cir_start_at_zero(hip, monkeypatch):
    """the reference asserts y0 > 0 and the one-launch kernel relies on it; a zero start routes the book to the interpreter kernel
    (as test_edge_cases.test_cir_intensity_starting_at_zero arranges), whose CIR++ root has the zero test"""
    from mcx.models.cirpp import CIRPPModel
    monkeypatch.setattr(CIRPPModel, "_initial_state", lambda self: [0.0, 0.0])
    ctl = _fused_controller("VAS_CIR_E", hip, 8)
    assert hip.sim_describe(ctl._sim)["signature"] == "VAS_CIR_E"
    _fused_runs(hip, ctl, "fused", 7, ("interpreter", "VAS_CIR_E"))
