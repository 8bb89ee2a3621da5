"""Sensitivities through the gas storage, host side (no GPU): the numpy restatement of the dual recursion
(tests/storage_tangent_reference.py) against the reference's autograd gradients (tests/golden/storage_*_aad.npz), the pieces the
restatement and the kernels share with the models (complex-safe closed forms, Cholesky tangents), the refusals and the ABI.

Bounds against the reference.  PV does not depend on coefficient tangents: 2e-6 max|row| + 1e-9, the bound the project holds
reference-autograd fixtures to (test_hip_parity.py).  Exposure-type metrics go through the derivative of the reference's lstsq on
raw monomials: where that bound is not met, the fixture records the measured restatement-against-reference error
(`reference_own_error_*`, written by gen_storage_aad_golden.py) and the bound is 4x the recorded value — the margin
test_storage_gpu.py gives `expo_own_error`.  Measured: 1.1e-8 / 1.7e-8 at degree 2 (storage_const, storage_short_last), 4.3e-6 at
degree 3 (storage_shift), 6.3e-6 for the EPE of storage_mixed's second netting set; storage_mixed's collateralised set (storage
+ European call netted, threshold 0.5, margin period 0.125, restated in storage_tangent_reference.restate_european /
unsecured_profile) 2.0e-7 for CVA and 1.8e-6 for EPE, so it is held to 2e-6; the restatement that differentiates
torch.linalg.lstsq on the raw system by reverse mode, as the reference does, moves by 3e-10 at degree 2 and 3e-5 .. 2e-4 at degree
3 against the centred solve (`raw_vs_centred_*`; it varies with torch's thread count), i.e. the gap to the reference is the size of
the raw solve's own conditioning, and PV — which no solve touches — agrees to 2e-16.  Every recorded error is far below 1e-3 of its
gradient row, so every pair pins its gradient — with one exception that no bound can mend: a storage's regressed exposure is
never negative in the three Schwartz two-factor cases, so their ENE values AND ENE gradient rows are identically zero in the
reference, in the restatement and on the GPU (recorded errors exactly 0.0).  Those ENE checks pin that the row stays zero and
nothing else; no case here exercises a negative-exposure tangent (storage_mixed, whose call could produce one, has no ENE metric).

The reference reports NO rho sensitivity under EULER (its correlation matrix is built at construction, off the tape): those fixture
entries are NaN and are skipped; the restatement's rho column is exact to rounding by construction (complex step)."""
import os
import re

import numpy as np
import pytest

import storage_cases
import storage_tangent_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PV_RTOL, PV_ATOL, OWN_ERROR_MARGIN = 2e-6, 1e-9, 4.0


def load_aad(name):
    return np.load(os.path.join(storage_cases.GOLDEN, name + "_aad.npz"))


def reference_bound(ga, tag, is_pv):
    """relative bound (of max|row|) of a gradient against the reference: 2e-6, or 4x the error MEASURED for this netting set and
    metric where that is larger.  Every (netting set, metric) of every case has a measured number — the restatement covers the
    collateralised set of storage_mixed (storage + European call, threshold, margin period) as well; a NaN would fail here."""
    if is_pv:
        return PV_RTOL
    own = float(ga["reference_own_error_" + tag])
    assert not np.isnan(own), ("no measured restatement-against-reference error", tag)
    return PV_RTOL if own <= PV_RTOL else OWN_ERROR_MARGIN * own


def check_against_reference(name, ga, tag, got, is_pv):
    ref = ga["grad_" + tag]
    have = ~np.isnan(ref)                                      # NaN: the reference reports no gradient (rho under EULER)
    scale = np.nanmax(np.abs(ref), axis=1, keepdims=True)
    tol = reference_bound(ga, tag, is_pv) * scale + PV_ATOL
    err = np.where(have, np.abs(got - np.where(have, ref, 0.0)), 0.0)
    print(name, tag, "max gradient error / max|row|", (err / np.maximum(scale, 1e-300)).max(), "bound", reference_bound(ga, tag, is_pv))
    assert got.shape == ref.shape and (err <= tol).all(), (name, tag, (err / tol).max())


@pytest.mark.parametrize("name", list(storage_cases.CASES))
def test_restatement_reproduces_the_reference_gradients(name):
    ga = load_aad(name)
    r = T.restate_case(name, centred=True)
    sc = r["sc"]
    assert len(r["grads"]) == len(sc.netting_sets) * len(sc.risk_metrics.metrics), "the restatement covers every netting set of every case"
    for tag, got in r["grads"].items():
        m_i = int(tag.split("_")[1])
        check_against_reference(name, ga, tag, got, sc.risk_metrics.metrics[m_i].get_name() == "pv")
    if name == "storage_short_last":                           # EULER: the reference has no rho gradient, ours is not zero
        assert np.isnan(ga["grad_0_0"][0, 5]) and abs(r["grads"]["0_0"][0, 5]) > 1e-3


@pytest.mark.parametrize("name", list(storage_cases.CASES))
def test_recorded_reference_errors_pin_the_gradients(name):
    """a metric / case pair whose recorded error exceeded 1e-3 of its gradient row would pin nothing"""
    ga = load_aad(name)
    keys = [k for k in ga.files if k.startswith("reference_own_error_")]
    assert keys and float(ga["reference_seconds"]) > 0.0
    assert len(keys) == len([k for k in ga.files if k.startswith("grad_")]), "every netting set and metric has a measured error"
    for k in keys:
        v = float(ga[k])
        assert v < 1e-3, (name, k, v)                              # (NaN fails: nothing is bounded by an unmeasured number)
        raw = float(ga["raw_vs_centred_" + k[len("reference_own_error_"):]])
        assert raw < 1e-3, (name, k, raw)


@pytest.mark.parametrize("name", list(storage_cases.CASES))
def test_path_restatement_reproduces_the_fixture_paths(name):
    """the step maps the complex step runs through give the reference's paths on its draws"""
    from mcx.common.enums import SimulationScheme
    from mcx.plan import SimPlan
    from test_storage_reference import compiled_controller
    sc, g = compiled_controller(name)
    _b, _n0, _n1, steps, scheme, _d = storage_cases.CASES[name]
    plan = SimPlan(sc.model, sc.simulation_timeline.numpy(), getattr(SimulationScheme, scheme), steps)
    for phase in ("pre", "main"):
        ours = np.transpose(T.restate_paths(sc.model, plan, g["z_" + phase]).real, (2, 0, 1))
        assert np.allclose(ours, g["paths_" + phase], rtol=1e-11, atol=1e-13), (name, phase, np.abs(ours - g["paths_" + phase]).max())


@pytest.mark.parametrize("scheme", ["EULER", "ANALYTICAL"])
def test_s2f_cholesky_closed_form_and_its_tangents(scheme):
    """_cholesky_entries equals the factor the path kernel is given, and its complex-step derivative equals central differences"""
    from mcx.common.enums import SimulationScheme
    sch = getattr(SimulationScheme, scheme)
    model = storage_cases._gas_model(storage_cases.mcx_classes())
    for dt in (0.5, 1.0, 2.0 / 3.0):
        L = np.array(model._cholesky_entries(sch, dt), dtype=np.float64)
        assert np.allclose(L, model.get_cholesky(sch, dt).numpy(), rtol=1e-14, atol=1e-16)
        for j in range(6):
            theta = float(model.model_params[j])
            h = 1e-30 * max(abs(theta), 1e-2)
            d_cs = np.imag(np.array(T.complex_model(model, j, h)._cholesky_entries(sch, dt), dtype=np.complex128)) / h
            e = 1e-6 * max(abs(theta), 1e-2)
            up, dn = T.complex_model(model, j, 0.0), T.complex_model(model, j, 0.0)
            up._complex_step[j], dn._complex_step[j] = complex(theta + e, 0.0), complex(theta - e, 0.0)
            d_fd = np.real(np.array(up._cholesky_entries(sch, dt), dtype=np.complex128) - np.array(dn._cholesky_entries(sch, dt), dtype=np.complex128)) / (2.0 * e)
            assert np.allclose(d_cs, d_fd, rtol=1e-6, atol=1e-9), (scheme, dt, j, d_cs, d_fd)
    if scheme == "EULER":
        d_rho = np.imag(np.array(T.complex_model(model, 5, 1e-30)._cholesky_entries(sch, None), dtype=np.complex128)) / 1e-30
        rho = float(model.model_params[5])
        assert np.allclose(d_rho, [[0.0, 0.0], [1.0, -rho / np.sqrt(1.0 - rho * rho)]], rtol=1e-14, atol=1e-16)


def test_dual_least_squares_against_central_differences():
    """lstsq_dual / solve_dual: the derivative of a regression whose matrix AND right-hand sides move"""
    rng = np.random.default_rng(5)
    n, K, S = 512, 4, 3
    x, dx = 30.0 * np.exp(0.1 * rng.normal(size=n)), rng.normal(size=(2, n))
    Y = np.stack([x ** 2 * 0.1 + rng.normal(size=n), x + rng.normal(size=n), rng.normal(size=n)], axis=1)
    dY = rng.normal(size=(2, n, S))
    c, dc = T.solve_dual(x, dx, Y, dY, K, centred=True)
    xs = np.linspace(x.min(), x.max(), 9)
    B = np.stack([xs ** k for k in range(K)], axis=1)
    for q in range(2):
        e = 1e-6
        up = np.linalg.lstsq(np.stack([((x + e * dx[q] - 30.0) / 5.0) ** k for k in range(K)], axis=1), Y + e * dY[q], rcond=None)[0]
        dn = np.linalg.lstsq(np.stack([((x - e * dx[q] - 30.0) / 5.0) ** k for k in range(K)], axis=1), Y - e * dY[q], rcond=None)[0]
        Bz = np.stack([((xs - 30.0) / 5.0) ** k for k in range(K)], axis=1)
        fd = Bz @ (up - dn) / (2.0 * e)                        # the fitted curves' derivative on a grid of x (basis-independent)
        assert np.allclose(B @ dc[q].T, fd, rtol=1e-5, atol=1e-6 * np.abs(fd).max()), (q, np.abs(B @ dc[q].T - fd).max())


# ---- refusals and ABI ------------------------------------------------------------------------------------------------------------
def test_oracle_backend_refuses_storage_sensitivities_at_construction():
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    from oracle_backend import OracleBackend
    ns, model, rm = storage_cases.storage_const(storage_cases.mcx_classes())
    with pytest.raises(NotImplementedError, match="storage policy"):
        SimulationController(ns, model, rm, 64, 64, 1, SimulationScheme.ANALYTICAL, True, backend=OracleBackend())


def test_a_backend_with_the_entry_points_constructs_and_refuses_what_forward_mode_cannot_do():
    """construction succeeds with a backend that has tangent_storage_eval; forward_mode = False and second order are refused with
    their reason before any kernel runs; nothing falls back to bump-and-revalue"""
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController

    class Stub:
        name = "stub"

        def tangent_storage_eval(self, *a, **k):
            raise AssertionError("not reached")

    def build():
        ns, model, rm = storage_cases.storage_const(storage_cases.mcx_classes())
        return SimulationController(ns, model, rm, 64, 64, 1, SimulationScheme.ANALYTICAL, True, backend=Stub())

    sc = build()
    sc.forward_mode = False
    with pytest.raises(NotImplementedError, match="storage policy.*forward_mode"):
        sc.run_simulation()
    sc = build()
    sc.compute_higher_derivatives()
    with pytest.raises(NotImplementedError, match="storage policy.*second-order"):
        sc.run_simulation()


@pytest.mark.parametrize("scheme", ["EULER", "ANALYTICAL"])
def test_s2f_dual_paths_are_for_books_that_hold_a_storage(scheme):
    """a Schwartz two-factor book without a storage never reaches tangent_paths_s2f: under ANALYTICAL run_with_tangent_book has no
    tangent form for it (as before the storage's sensitivities existed), under EULER it goes on to tangent_paths, which the library
    answers with MCX_E_NOT_FUSABLE for this model"""
    import cases
    from mcx import aad
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    reached = []

    class Stub:
        name = "stub"

        def tangent_paths_s2f(self, *a, **k):
            reached.append("s2f")
            raise AssertionError("reached")

        def tangent_storage_eval(self, *a, **k):
            raise AssertionError("reached")

    ns, model, rm = cases.s2f_european()
    sc = SimulationController(ns, model, rm, 64, 0, 1, getattr(SimulationScheme, scheme), True, backend=Stub())
    if scheme == "ANALYTICAL":
        with pytest.raises(aad._NoTangentForm, match="scheme"):
            aad.run_with_tangent_book(sc)
    else:
        with pytest.raises(Exception) as e:                            # the stub has no kernels: whatever fails first, it is not s2f
            aad.run_with_tangent_book(sc)
        assert not isinstance(e.value, AssertionError), e.value
    assert not reached


def test_new_entry_points_are_declared_and_exported():
    from mcx import _native
    text = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for sym in ("mcx_tangent_storage_lsm_step", "mcx_tangent_storage_eval", "mcx_tangent_paths_s2f"):
        assert re.search(r"^int\s+" + sym + r"\s*\(", text, flags=re.M), sym
        assert sym in _native._EXPORTS
    assert re.search(r"#define MCX_ABI_VERSION 6\b", text)
    for method in ("tangent_storage_lsm_step", "tangent_storage_eval", "tangent_paths_s2f"):
        assert callable(getattr(_native.HipBackend, method))
