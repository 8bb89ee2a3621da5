"""Forward-mode sensitivities of wide models, host side (no GPU): the numpy restatement with explicit tangents against differences
of the primal restatement, the gate mcx.aad.wide_route, the active-slot derivation.

The restatement's tangents (tests/wide_tangent_reference.py) are compared with 4-point central differences of the PRIMAL recursion
of tests/wide_paths_reference.py, run in long double on tables moved along the derivative tables' direction.  That recursion takes
its tables as doubles, so a table entry t moved by s h d carries a rounding error of 1.1e-16 |t|, which reaches a row of paths in proportion to the row's value: the
difference quotient of a row f is off by up to 64 (18 / 12) 1.1e-16 max|f| / h (at most 64 entries enter a row), plus the formula's
truncation, of order (2^-10)^4 of the tangent row for a step h of 2^-10 of the entries that move.  The bound is their sum per row
(date, state column); the measured gap is printed, also relative to the tangent row's largest entry."""
import types

import numpy as np
import pytest

import cases
import wide_cases as wc
import wide_paths_reference as wr
import wide_tangent_reference as wt
from mcx import _abi, aad
from mcx.common.enums import SimulationScheme

NP = _abi.TANGENT_NP
STEP = 2.0 ** -10


def _moved(plan, d, q, s):
    """a plan-like object whose tables are plan's + s d[..., q] (what wide_paths_reference.run reads)"""
    recs = []
    for i, sl in enumerate(wr.slot_records(plan)):
        recs.append(types.SimpleNamespace(kind=sl["kind"], state_off=sl["state_off"], p=[sl["p"][j] + s * d["slots"][i, j, q] for j in range(8)]))
    chol = plan.chol + (s * d["chol"][..., q] if d["chol"] is not None else 0.0)
    return types.SimpleNamespace(wide=True, slot_records=recs, n_slots=plan.n_slots, desc=plan.desc, n_dates=plan.n_dates,
                                 n_state=plan.n_state, n_initial_store=plan.n_initial_store, n_steps=plan.n_steps, steps=plan.steps,
                                 init_state=plan.init_state + s * d["init"][:, q], chol=chol, aux=plan.aux + s * d["aux"][..., q])


@pytest.mark.parametrize("name,build,scheme", [
    ("vbcd_9_euler", lambda: wc.mixed_model("VBCDVBCDV", 42), "EULER"),
    ("bs_12_analytical", lambda: wc.bs_multi(12, 25), "ANALYTICAL"),
])
def test_restatement_against_differences_of_the_primal_recursion(name, build, scheme):
    from mcx.plan import SimPlan
    model = build()
    plan = SimPlan(model, wc.TIMELINE, SimulationScheme[scheme], wc.NUM_STEPS)
    dd = wt.derivative_tables(model, plan)
    z = np.random.default_rng(2).standard_normal((plan.n_steps, plan.n_z, 33))
    worst = rel = 0.0
    for sel, d in wt.chunks(dd, len(model.get_model_params()), NP):
        hi = wt.run(plan, z, d["slots"], d["init"], d["aux"], d["chol"], wt.LD)
        assert hi.min_floor_gap > 1e-3
        assert np.array_equal(hi.paths, wr.run(plan, z, wt.LD).paths), "the value rows are the primal restatement's"
        for q in range(len(sel)):
            # the step: 2^-10 of the smallest ratio |table entry| / |its derivative| over the entries that move
            ratios = []
            tabs = [(np.array([sl["p"] for sl in wr.slot_records(plan)]), d["slots"][..., q]), (plan.init_state, d["init"][:, q]), (plan.aux, d["aux"][..., q])]
            if d["chol"] is not None:
                tabs.append((plan.chol, d["chol"][..., q]))
            for t0, dq in tabs:
                m = (dq != 0) & (np.abs(t0) > 1e-8)      # (entries that are zero up to rounding, psi(t) of CIR++, enter linearly)
                if m.any():
                    ratios.append(np.min(np.abs(t0[m] / dq[m])))
            if not any(dq.any() for _t0, dq in tabs):           # a parameter no table depends on (deterministic credit)
                assert not hi.dpaths[q].any()
                continue
            h = STEP * min(ratios) if ratios else STEP * 1e-3   # (only near-zero entries move: an absolute step of their size)
            f = {s: wr.run(_moved(plan, d, q, s * h), z, wt.LD).paths for s in (1, -1, 2, -2)}
            fd = (8 * (f[1] - f[-1]) - (f[2] - f[-2])) / (12 * wt.LD(h))
            scale = np.abs(hi.dpaths[q]).max(axis=-1)
            gap = np.abs(fd - hi.dpaths[q]).max(axis=-1)
            # per row (date, state column): the rounding of the moved tables scales with the row's VALUE over the step (a tangent row
            # may be a small residual: d Lambda / d kappa of CIR++ started at y0 = theta), the truncation with the tangent itself
            tol = 64 * 1.5 * 1.1e-16 * np.abs(f[1]).max(axis=-1) / h + STEP ** 4 * scale
            assert not ((tol == 0) & (gap > 0)).any()
            worst = max(worst, float(np.max(gap / np.where(tol == 0, 1, tol))))
            rel = max(rel, float(np.max(gap / np.where(scale == 0, 1, scale))))
    print(f"WIDE-TANGENT host {name}: restatement against 4-point differences, worst gap / bound {worst:.3e}; "
          f"worst gap / row's largest entry {rel:.3e}")
    assert worst <= 1.0


def _fake(model, scheme="EULER", flag=True, binding=True, products=()):
    be = types.SimpleNamespace(tangent_paths_wide=None) if binding else types.SimpleNamespace()
    return types.SimpleNamespace(tangent_wide=flag, backend=be, model=model, simulation_scheme=SimulationScheme[scheme], products=list(products))


def _slots_model(specs):
    return types.SimpleNamespace(_slots=lambda: specs)


def test_wide_route_truth_table():
    mix = lambda n: wc.mixed_model("".join("VBCD"[k % 4] for k in range(n)), 3)
    assert aad.TANGENT_MAX_SLOTS == 4
    for n, want in ((4, False), (5, True), (8, True), (9, True), (32, True)):
        assert aad.wide_route(_fake(mix(n))) is want, n
    assert not aad.wide_route(_fake(mix(9), flag=False))
    assert not aad.wide_route(_fake(mix(9), binding=False))
    assert not aad.wide_route(_fake(wc.mixed_model("VBCHDVBCD", 3)))                      # a Hull-White slot
    assert not aad.wide_route(_fake(wc.mixed_model("VBHBB", 3)))
    two = [types.SimpleNamespace(sim_dim=2, kind=_abi.MODEL_BS)] + [types.SimpleNamespace(sim_dim=1, kind=_abi.MODEL_BS)] * 5
    assert not aad.wide_route(_fake(_slots_model(two)))                                   # a two-factor leaf
    assert aad.wide_route(_fake(_slots_model(two[1:])))
    assert not aad.wide_route(_fake(wc.bs_multi(12, 1), scheme="QE"))
    assert aad.wide_route(_fake(wc.bs_multi(12, 1), scheme="ANALYTICAL")) and aad.wide_route(_fake(wc.bs_multi(12, 1)))
    assert not aad.wide_route(_fake(mix(9), scheme="ANALYTICAL"))                         # CIR++ has no analytic tangent step
    assert not aad.wide_route(_fake(mix(9), products=[types.SimpleNamespace(is_storage=True)]))
    assert aad.wide_route(_fake(mix(9), products=[types.SimpleNamespace()]))


def test_flag_off_keeps_the_gates_and_flag_on_opens_them(oracle):
    from mcx.controller.controller import SimulationController
    sc, _ = wc.make_controller("wide_basket12_analytical_aad", oracle, inject=False)
    assert sc.tangent_wide is False and sc._force_wide_plan is False
    with pytest.raises(aad._NoTangentForm, match="wide model"):
        aad._tangent_book_routes(sc)
    sc.tangent_wide = True                                     # the oracle backend has no binding: the fallback stays
    with pytest.raises(aad._NoTangentForm, match="wide model"):
        aad._tangent_book_routes(sc)
    oracle.tangent_paths_wide = oracle.tangent_paths_chol = None
    try:
        assert aad.wide_route(sc) and not aad.payoff_forms_armed(sc, oracle)
        s2f, chol, batched = aad._tangent_book_routes(sc)     # every later gate passes too: the book takes the forward pass
        assert (s2f, bool(chol), batched) == (False, True, False)
    finally:
        del oracle.tangent_paths_wide, oracle.tangent_paths_chol
    assert aad._clone_controller(sc, sc.model, True)._force_wide_plan is False
    assert aad._clone_controller(sc, sc.model, True, force_wide=True)._force_wide_plan is True
    assert isinstance(sc, SimulationController) and aad._BookPass._fields[-2:] == ("wide", "active")


def test_active_slots_on_hand_made_tables():
    plan = types.SimpleNamespace(slot_states=[(0, 1), (1, 2), (3, 2), (5, 1)])
    z = lambda *s: np.zeros(s + (NP,))
    dslot, dinit, daux, dchol = z(4, 8), z(6), z(3, 4, 8), z(2, 4, 4)
    assert aad.active_slots(plan, dslot, dinit, daux) == [] == aad.active_slots(plan, dslot, dinit, daux, dchol)
    dslot[2, 7, 3] = 1e-300
    assert aad.active_slots(plan, dslot, dinit, daux) == [2]
    dinit[2, 0] = -1.0                                         # the second state row of slot 1
    assert aad.active_slots(plan, dslot, dinit, daux) == [1, 2]
    daux[2, 0, 5, 1] = 2.0                                     # the last sub-step of slot 0
    assert aad.active_slots(plan, dslot, dinit, daux) == [0, 1, 2]
    dchol[1, 3, 0, 2] = 1.0                                    # row 3 of the second factor: read under ANALYTICAL only
    assert aad.active_slots(plan, dslot, dinit, daux) == [0, 1, 2]
    assert aad.active_slots(plan, dslot, dinit, daux, dchol) == [0, 1, 2, 3]
    dchol[:] = 0.0
    dchol[0, 0, 3, 0] = 1.0                                    # COLUMN 3 of row 0: slot 0's, not slot 3's
    assert aad.active_slots(plan, dslot, dinit, daux, dchol) == [0, 1, 2]
    # and on a real plan, against the derivation of the test reference
    model = wc.bs_multi(12, 25)
    real = wc.plan_of("bs_12_analytical")
    dd = wt.derivative_tables(model, real)
    for sel, d in wt.chunks(dd, len(model.get_model_params()), NP):
        assert aad.active_slots(real, d["slots"], d["init"], d["aux"], d["chol"]) == wt.active_from_tables(real, d["slots"], d["init"], d["aux"], d["chol"])
