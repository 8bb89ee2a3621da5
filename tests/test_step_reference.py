"""The long-double step reference (step_reference.py) and its harness are right — CPU only.

a. the reference reproduces the step maps recorded from the reference project (tests/golden/steps.npz) within its own bound at
   u = 2^-52;
b. the oracle backend goes through the harness of test_step_kernels.py on the same cases and shapes, with injected draws
   throughout (the oracle has no draw helper: on the Philox draws there is nothing for it to check), and every entry lies within
   the bound at u = 2^-52 — a ratio above 1 means a missing hook or a wrong formula in the reference;
c. the harness fails on the committed inputs when the reference is replaced by each subtly wrong map of step_reference.MUTATIONS;
d. the caps the GPU suite asserts hold for the oracle's own states, and the QE sets are what they were chosen for."""
import os

import numpy as np
import pytest

import cases
import step_cases as sc
import step_reference as sr
from mcx.models.black_scholes import BlackScholesModel
from mcx.models.cirpp import CIRPPModel
from mcx.models.heston import HestonModel
from mcx.models.vasicek import VasicekModel
from mcx.plan import SimPlan

G = np.load(os.path.join(cases.GOLDEN, "steps.npz"))


def _golden_plan(model, scheme):
    """the one sub-step [t1, t2] of the fixture with the model's own factor (as test_oracle_units._one_step builds it)"""
    t1, t2 = float(G["t1"][0]), float(G["t2"][0])
    plan = SimPlan(model, np.array([t2]), scheme, 1)
    dt = t2 - t1
    plan.steps["dt"], plan.steps["sqrt_dt"], plan.steps["t1"] = dt, np.sqrt(dt), t1
    plan.aux[:] = 0
    for s, vals in enumerate(model._step_aux(scheme, t1, dt)):
        plan.aux[0, s, :len(vals)] = vals
    plan.chol[0] = model.get_cholesky(scheme, dt).numpy()
    return plan


def test_reference_reproduces_the_recorded_step_maps():
    he = HestonModel(0.0, 800.0, 0.04, 0.45545583, -0.78975708, 0.01713417, 2.0, 0.0286834)
    he2 = HestonModel(0.0, 100.0, 0.02, 1.2, -0.5, 0.5, 0.02, 0.02)
    bs = BlackScholesModel(0.0, 120.0, 0.05, 0.2)
    va = VasicekModel(0.0, 0.03, 0.05, 0.1, 0.01, asset_id="irs")
    ci = CIRPPModel(0.0, "cp", cases.HAZARDS, 0.1, 0.01, 0.02, 1e-4)
    cd = CIRPPModel(0.0, "cp", cases.HAZARDS, 0.1, 0.01, 0.02, 1e-4, deterministic=True)
    rows = [(bs, sc.A, "bs_state", "bs_z", None, "bs_exact", False), (bs, sc.E, "bs_state", "bs_z", None, "bs_euler", False),
            (va, sc.A, "va_state", "va_z", None, "va_exact", False), (va, sc.E, "va_state", "va_z", None, "va_euler", False),
            (ci, sc.E, "ci_state", "ci_z", None, "ci_euler", False), (cd, sc.E, "ci_state", "ci_z", None, "cd_euler", False),
            (he, sc.E, "he_state", "he_z", None, "he_euler", False),
            (he, sc.Q, "he_state", "he_z", "he_qe_hard_u", "he_qe_hard", False), (he, sc.Q, "he_state", "he_z", "he_qe_fuzzy_u", "he_qe_fuzzy", True),
            (he2, sc.Q, "he2_state", "he_z", "he2_qe_hard_u", "he2_qe_hard", False), (he2, sc.Q, "he2_state", "he_z", "he2_qe_fuzzy_u", "he2_qe_fuzzy", True)]
    for model, scheme, st, z, u, want, smooth in rows:
        model.perform_smoothing = smooth
        tb = sr.Tables(_golden_plan(model, scheme))
        paths = np.stack([G[st].T, G[want].T])                  # [2 dates][n_state][n]: the recorded state before and after
        uu = G[u][:, 0] if u else None
        rep = sr.check_paths(tb, paths, lambda k: (G[z].T, uu), sr.U_IEEE, transitions=[(0, 1, 0, 1)])
        print(want, rep)
        rep.assert_ok(want)
        if scheme == sc.Q:
            assert rep.near_branch == 0 and rep.ill_conditioned == 0, (want, str(rep))


_RUNS = {}


def _oracle_run(oracle, key, model, scheme, nsub, n, seed, edges):
    if key not in _RUNS:
        _RUNS[key] = sc.run_injected(oracle, model, scheme, nsub, n, seed, edges=edges)
    return _RUNS[key]


def _injected_run(oracle, case, n=sc.N):
    return _oracle_run(oracle, ("inj", case[0], n), sc.build_model(case), case[2], case[3], n, case[4], True)


@pytest.mark.parametrize("case", sc.INJECTED + sc.INJECTED_SPECIAL, ids=lambda c: c[0])
def test_oracle_within_bound_on_the_injected_cases(case, oracle):
    """start states per path, edge states in the first block(s), every one of the twelve maps but QE (below)"""
    run = _injected_run(oracle, case)
    rep = sr.check_paths(run.tb, run.paths, run.draws, sr.U_IEEE)
    print(case[0], rep)
    rep.assert_ok(case[0])
    if case[0] == "cirpp-euler-floor":
        assert int((run.paths[1, 0, :run.n_edge] == 1e-12).sum()) >= run.n_edge // 30, str(rep)      # z = -8.5 from y = 0.05, every 30th edge path: the floor engages


@pytest.mark.parametrize("case", sc.PHILOX, ids=lambda c: c[0])
def test_oracle_within_bound_on_the_philox_cases(case, oracle):
    """the models of the Philox routes from the model's own start state (injected normals here)"""
    run = _oracle_run(oracle, ("phi", case[0]), sc.build_model(case), case[2], case[3], sc.N, case[4], False)
    rep = sr.check_paths(run.tb, run.paths, run.draws, sr.U_IEEE)
    print(case[0], rep)
    rep.assert_ok(case[0])


def test_oracle_within_bound_at_63_paths(oracle):
    case = sc.INJECTED[0]
    rep = sr.check_paths(*(lambda r: (r.tb, r.paths, r.draws))(_injected_run(oracle, case, 63)), sr.U_IEEE)
    rep.assert_ok(case[0])


def _qe_run(oracle, case, nsub, smooth, edges):
    return _oracle_run(oracle, ("qe", case, nsub, smooth, edges), sc.heston_qe(case, smooth), sc.Q, nsub, sc.N, 300 + case, edges)


QE_ALL = [(c, n, False) for v in sc.QE_HARD.values() for c, n in v] + [(sc.QE_CAP, 1, False)] + [(c, n, True) for c, n in sc.QE_SMOOTH]


@pytest.mark.parametrize("case,nsub,smooth", QE_ALL, ids=[f"{'smooth' if s else 'hard'}-{c}-{n}" for c, n, s in QE_ALL])
def test_oracle_within_bound_on_the_qe_sets(case, nsub, smooth, oracle):
    """with the edge states (v from 0 to 10 and at psi = 1, 1.5, 2; u at both ends and at p; z1 = +-8.5 and -b), and d. the caps:
    the same run at the kernels' u = 2^-50 leaves out no path-step in the hard regime and at most 1e-3 in the smoothed one.
    Measured on the oracle: near-branch 0 of 16388 .. 49164 path-steps for every hard set; ill-conditioned 0 for every smoothed
    set (sets 1, 7, 14, 21: 0 of 15650, 13485, 14352 and 47076 finite path-steps)."""
    run = _qe_run(oracle, case, nsub, smooth, True)
    capped = sr.check_paths(run.tb, run.paths, run.draws, sr.U_KERNEL, n_edge=run.n_edge)
    print(case, nsub, smooth, capped)
    capped.assert_ok((case, nsub, smooth))
    # (the bound is linear in u: within it at u = 2^-52 is a ratio of at most 1/4 at u = 2^-50)
    assert max(capped.worst.values()) <= sr.U_IEEE / sr.U_KERNEL, str(capped)
    assert capped.near_branch == 0, str(capped)
    assert capped.ill_conditioned <= 1e-3 * capped.finite_path_steps, str(capped)
    if smooth:
        assert capped.nan_entries > 0, "a smoothed set is chosen because its variance goes negative"


def test_qe_sets_are_what_they_are_chosen_for(oracle):
    """at least two all-quadratic, two all-tail and three mixed sets (5-95 % of the path-steps on each side of psi = 1.5) in the hard
    regime, on the oracle's own states from the model's start state"""
    share = {}
    for kind, sets in sc.QE_HARD.items():
        for case, nsub in sets:
            run = _qe_run(oracle, case, nsub, False, False)
            tail = tot = 0
            for d0, d1, k0, ns in run.tb.transitions():
                dr = [run.draws(k0 + j) for j in range(ns)]
                a = sr.advance(run.tb, k0, ns, run.paths[d0], [d[0] for d in dr], [d[1] for d in dr], bound=False)
                tail += int((a.mon["margin_psi"] > 0).sum())
                tot += a.mon["margin_psi"].size
            share[(kind, case)] = tail / tot
    print(share)
    assert sum(v == 0.0 for (k, _), v in share.items() if k == "quadratic") >= 2
    assert sum(v == 1.0 for (k, _), v in share.items() if k == "tail") >= 2
    assert sum(0.05 <= v <= 0.95 for (k, _), v in share.items() if k == "mixed") >= 3
    assert len({c for v in sc.QE_HARD.values() for c, _ in v}) == 8 and len(sc.QE_SMOOTH) == 4


# c. every mutation on a case whose inputs reach what it breaks
MUTATION_CASES = {
    "psi_eps": ("qe", 1, 1, True), "omu_floor": ("qe", 9, 1, False), "p_cap": ("qe", sc.QE_CAP, 1, False), "k1_k2": ("qe", 3, 1, False),
    "right_endpoint": ("inj", "vasicek-euler-0"), "cir_floor": ("inj", "cirpp-euler-floor"), "sqrt_abs": ("inj", "cirpp-euler-2"),
    "chol_transposed": ("phi", "multi-analytical-0"), "aux_next": ("inj", "bs-analytical-0"), "column_1e-13": ("inj", "hull_white-analytical-0"),
}


@pytest.mark.parametrize("mut", sr.MUTATIONS)
def test_harness_detects_a_subtly_wrong_map(mut, oracle):
    spec = MUTATION_CASES[mut]
    if spec[0] == "qe":
        run = _qe_run(oracle, spec[1], spec[2], spec[3], True)
    elif spec[0] == "inj":
        run = _injected_run(oracle, next(c for c in sc.INJECTED + sc.INJECTED_SPECIAL if c[0] == spec[1]))
    else:
        case = next(c for c in sc.PHILOX if c[0] == spec[1])
        run = _oracle_run(oracle, ("phi", case[0]), sc.build_model(case), case[2], case[3], sc.N, case[4], False)
    sr.check_paths(run.tb, run.paths, run.draws, sr.U_KERNEL, n_edge=run.n_edge).assert_ok((mut, "unmutated"))
    rep = sr.check_paths(run.tb, run.paths, run.draws, sr.U_KERNEL, mut=mut, n_edge=run.n_edge)
    print(mut, len(rep.failures), rep)
    assert rep.failures, f"the harness did not notice the mutation {mut}"


@pytest.mark.parametrize("mut,also", [("right_endpoint", ["hull_white-euler-0", "cirpp-euler-1"]), ("sqrt_abs", ["heston-euler-0"])])
def test_harness_detects_the_mutation_in_every_map_it_touches(mut, also, oracle):
    for name in also:
        run = _injected_run(oracle, next(c for c in sc.INJECTED if c[0] == name))
        assert sr.check_paths(run.tb, run.paths, run.draws, sr.U_KERNEL, mut=mut).failures, (mut, name)


def test_host_draws_are_the_oracles(oracle):
    """step_cases.host_draws (the draws behind the allowance of test_hip_parity.test_heston_qe_random_parameters_gpu_vs_oracle) against
    orc_draw, counter by counter: the uniforms bit for bit, the normals within 4 ulp of libm's, also from path 2^33 + 12345"""
    import ctypes as C
    plan = SimPlan(sc.heston_qe(3, False), np.array([0.5, 1.0]), sc.Q, 3)
    n = 48
    for off in (0, sc.OFFSET_BIG):
        draws = sc.host_draws(plan, 43, off, n)
        for k in (0, 4):
            z, u = draws(k)
            for i in range(n):
                got = [C.c_double() for _ in range(8)]
                for q in (0, 1):
                    oracle.lib.orc_draw(C.c_uint64(43), C.c_uint64(off + i), C.c_uint32(k), C.c_uint32(q), *[C.byref(g) for g in got[4 * q:4 * q + 4]])
                assert u[i] == got[4].value, (off, k, i)
                for mine, ref in ((z[0, i], got[2].value), (z[1, i], got[3].value)):
                    assert abs(mine - ref) <= 4 * np.spacing(abs(ref)), (off, k, i, mine, ref)
