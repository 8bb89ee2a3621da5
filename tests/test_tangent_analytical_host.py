"""Forward-mode sensitivities under the ANALYTICAL scheme, the host side (no GPU): the closed-form Cholesky factor entries of the
models and their complex-step derivatives against torch.autograd through torch.linalg.cholesky, the factor block of the host
descriptors, the gate of run_with_tangent_book with stub backends, the new symbol, and the fixtures recorded from the reference
against the oracle backend's bump route."""
import copy
import os
import re
import types

import numpy as np
import pytest
import torch

import analytical_aad_cases as aad_cases
import cases
from mcx import aad
from mcx.plan import SimPlan
from test_oracle_golden import check_lsm_sensitivities

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO3 = [[1, .5, -.2], [.5, 1, .3], [-.2, .3, 1]]
RHO4_PAIRS = [0.5, 0.3, -0.2, 0.1, 0.4, 0.6]                                  # (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
TIMELINE = np.array([0.0, 0.25, 1.0])                                         # two sub-steps per interval: dt = 0.125 and 0.375


def _config4():
    models = [cases.BlackScholesModel(0.0, 100.0 + 5 * i, 0.01 * i, 0.2 + 0.1 * i, asset_id=f"a{i}") for i in range(4)]
    return cases.ModelConfig(models, inter_asset_correlation_matrix=np.array([[r] for r in RHO4_PAIRS]))


def _rho4():
    rho, k = np.eye(4), 0
    for i in range(4):
        for j in range(i + 1, 4):
            rho[i, j] = rho[j, i] = RHO4_PAIRS[k]
            k += 1
    return rho


# model, and the covariance of one step rebuilt in torch from the parameter tensors `th` (gradient order) and dt
MODELS = {
    "black_scholes": (lambda: cases.BlackScholesModel(0.0, 100.0, 0.03, 0.25), lambda th, dt: (th[1] * th[1] * dt).reshape(1, 1)),
    "vasicek": (lambda: cases.VasicekModel(0.0, 0.02, 0.04, 0.3, 0.015, asset_id="r"),
                lambda th, dt: ((th[1] ** 2 / (2 * th[3])) * (1 - torch.exp(-th[3] * dt) ** 2)).reshape(1, 1)),
    "multi3": (lambda: cases.BlackScholesMulti(0.0, 0.02, ["a1", "a2", "a3"], [100, 105, 95], [0.4, 0.3, 0.25], RHO3),
               lambda th, dt: torch.diag(torch.stack(th[3:6])) @ torch.tensor(RHO3, dtype=torch.float64) @ torch.diag(torch.stack(th[3:6])) * dt),
    "config4": (_config4, lambda th, dt: torch.diag(torch.stack(th[1::3])) @ torch.tensor(_rho4()) @ torch.diag(torch.stack(th[1::3])) * dt),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_factor_entries_and_their_derivatives_against_autograd(name):
    """closed form = the factor the path kernel is given (plan.chol); complex step = autograd through torch.linalg.cholesky.  Both
    at 1e-12 of the entry.  Entries whose derivative is exactly zero (the rows a volatility does not scale) come back from
    autograd's triangular solves as rounding noise of a few eps times the largest entry (measured 3.7e-16 against 0.35): the
    floor under the relative bound is 1e-14 of the largest entry, ~50 eps, the reference's own error and no more."""
    build, cov = MODELS[name]
    model = build()
    plan = SimPlan(model, TIMELINE, cases.A, 2)
    assert len(plan.chol) == 2 and plan.chol.shape[1:] == (plan.n_z, plan.n_z) == (len(model._slots()),) * 2
    P = len(model.get_model_params())
    for L_plan, dt in zip(plan.chol, plan.chol_dt):
        L = np.array(model._analytic_factor_entries(dt), dtype=np.float64)
        assert np.allclose(L, L_plan, rtol=1e-12, atol=1e-12 * np.abs(L_plan).max()), (name, dt, np.abs(L - L_plan).max())
        th = [torch.tensor(float(p.detach()), dtype=torch.float64, requires_grad=True) for p in model.get_model_params()]
        L_t = torch.linalg.cholesky(cov(th, dt))
        assert np.allclose(L_t.detach().numpy(), L_plan, rtol=1e-12, atol=1e-12 * np.abs(L_plan).max())
        d_ag = np.zeros(L.shape + (P,))
        for r in range(L.shape[0]):
            for c in range(r + 1):
                g = torch.autograd.grad(L_t[r, c], th, retain_graph=True, allow_unused=True)
                d_ag[r, c] = [0.0 if x is None else float(x) for x in g]
        assert np.abs(d_ag).max() > 0.0
        for j in range(P):
            m = copy.deepcopy(model)
            h = 1e-30 * max(abs(float(th[j].detach())), 1e-2)
            aad._set_complex_step(m, j, h)
            d_cs = np.imag(np.array(m._analytic_factor_entries(dt), dtype=np.complex128)) / h
            gap = np.abs(d_cs - d_ag[..., j])
            assert np.all(gap <= 1e-12 * np.abs(d_ag[..., j]) + 1e-14 * np.abs(d_ag[..., j]).max()), (name, dt, j, gap.max())


def test_a_config_without_a_closed_form_says_so():
    mixed = cases.irs_models(0.5)                                             # Vasicek + CIR++: no joint analytic covariance at all
    assert mixed._analytic_factor_entries(0.25) is None
    assert not aad._analytic_factor_form(mixed, cases.A)
    single = cases.ModelConfig([cases.VasicekModel(0.0, 0.02, 0.04, 0.3, 0.015, asset_id="r")])
    assert np.allclose(single._analytic_factor_entries(0.25), single.models[0]._analytic_factor_entries(0.25), rtol=0, atol=0)
    assert aad._analytic_factor_form(single, cases.A) and not aad._analytic_factor_form(single, cases.E)


def test_host_descriptors_carry_the_factor_block(oracle):
    """d["chol"] [n_chol][n_z][n_z] of a compiled controller whose timeline has distinct step lengths, equal to plan.chol; complex
    evaluation keeps the shape; under EULER there is no such block (the factor is parameter-free)"""
    ns, model, rm = aad_cases.basket3_multi()
    sc = cases.SimulationController(ns, model, rm, 64, 64, 2, cases.A, backend=oracle)
    sc.run_simulation()
    d, _ = aad._host_descriptors(sc)
    plan = sc.sim_plan
    assert len(plan.chol) >= 2 and d["chol"].shape == plan.chol.shape == (len(plan.chol), 3, 3)
    assert np.allclose(d["chol"], plan.chol, rtol=1e-12, atol=1e-14)
    m = copy.deepcopy(model)
    aad._set_complex_step(m, 3, 1e-30)                                        # volatility of the first asset: row 0 of every factor
    dc, _ = aad._host_descriptors(sc, m, dtype=np.complex128)
    assert dc["chol"].shape == d["chol"].shape
    assert np.allclose(dc["chol"].imag[:, 0, 0] / 1e-30, np.sqrt(np.array(plan.chol_dt)), rtol=1e-14)
    assert np.all(dc["chol"].imag[:, 1:, :] == 0.0)
    ns, model, rm = aad_cases.basket3_multi()
    se = cases.SimulationController(ns, model, rm, 64, 64, 2, cases.E, backend=oracle)
    se.run_simulation()
    assert "chol" not in aad._host_descriptors(se)[0]


# ---- the gate ------------------------------------------------------------------------------------------------------------------------
class _StubWithoutChol:
    name = "stub"

    def tangent_paths(self, *a, **k):
        raise AssertionError("reached")


class _StubWithChol(_StubWithoutChol):
    def tangent_paths_chol(self, *a, **k):
        raise AssertionError("reached")

    def tangent_lsm_step(self, *a, **k):
        raise AssertionError("reached")


def _controller(ns, model, rm, backend, n_pre=0):
    return cases.SimulationController(ns, model, rm, 64, n_pre, 1, cases.A, True, backend=backend)


def test_gate_without_the_entry_point_has_no_tangent_form():
    with pytest.raises(aad._NoTangentForm, match="scheme"):
        aad.run_with_tangent_book(_controller(*cases.american(), _StubWithoutChol(), 64))


def test_gate_with_the_entry_point_lets_black_scholes_and_vasicek_pass():
    for build in (cases.american, cases.bond_option, aad_cases.basket3_multi):
        with pytest.raises(Exception) as e:                                   # the stub has no kernels: whatever fails first is not the gate
            aad.run_with_tangent_book(_controller(*build(), _StubWithChol(), 64))
        assert not isinstance(e.value, (aad._NoTangentForm, AssertionError)), (build.__name__, e.value)


def test_gate_refuses_heston_and_hull_white_leaves_under_analytical():
    from test_hull_white import _hw
    hw = _hw()
    bond = cases.Bond(0.0, 1.0, 1.0, 0.5, True, 0.03, hw.asset_ids[0])
    sc = _controller([cases.NettingSet(name="b", products=[bond])], hw, cases.RiskMetrics([cases.PVMetric()]), _StubWithChol())
    assert not aad._analytic_factor_form(hw, cases.A)
    with pytest.raises(aad._NoTangentForm, match="scheme"):
        aad.run_with_tangent_book(sc)
    ns, heston, rm = cases.heston()
    assert not aad._analytic_factor_form(heston, cases.A)
    with pytest.raises(aad._NoTangentForm, match="scheme"):                   # (the gate comes before the plan, which Heston has none of here)
        aad.run_with_tangent_book(_controller(ns, heston, rm, _StubWithChol()))
    # a Heston leaf next to Black-Scholes ones
    mixed = cases.ModelConfig([cases.BlackScholesModel(0.0, 100.0, 0.03, 0.2, asset_id="a"),
                               cases.HestonModel(0.0, 100.0, 0.03, 0.4, -0.5, 1.0, 0.04, 0.04, asset_id="h")])
    assert not aad._analytic_factor_form(mixed, cases.A)


def test_the_symbol_is_declared_exported_and_bound():
    from mcx import _native
    text = open(os.path.join(ROOT, "include", "mcx.h")).read()
    assert re.search(r"^int\s+mcx_tangent_paths_chol\s*\(", text, flags=re.M)
    assert "mcx_tangent_paths_chol" in _native._EXPORTS and hasattr(_native.HipBackend, "tangent_paths_chol")
    assert re.search(r"#define MCX_ABI_VERSION 6\b", text)


# ---- the fixtures: the oracle backend's bump route meets the reference's autograd ------------------------------------------------------
@pytest.mark.parametrize("name", ["netting_aad", "bond_option_aad", "flexicall_aad"])
def test_oracle_bump_route_meets_the_fixture(name, oracle):
    sc, g = aad_cases.make_controller(name, oracle)
    res = sc.run_simulation()
    assert sc.timings["tangent"] is False                                     # the oracle has no dual kernels: bump-and-revalue
    check_lsm_sensitivities(sc, g, res)


def test_oracle_bump_route_meets_the_pv_rows_of_basket3_multi(oracle):
    """the EPE rows are not asked of the bump route: on one entry a bumped path crosses the exposure kink, an artefact of bumping
    (the reference's autograd is the yardstick there; the GPU test holds the forward pass to all rows)"""
    sc, g = aad_cases.make_controller("basket3_multi_aad", oracle)
    res = sc.run_simulation()
    assert list(g["metric_names"])[0] == res.metric_names[0] and len(res.results) == 2
    pv = types.SimpleNamespace(model_param_names=res.model_param_names, results=[[ns[0]] for ns in res.results],
                               derivatives=[[ns[0]] for ns in res.derivatives])
    g_pv = {"param_names": g["param_names"], **{f"{k}_{ns_i}_0": g[f"{k}_{ns_i}_0"] for k in ("result", "grad") for ns_i in range(2)}}
    check_lsm_sensitivities(sc, g_pv, pv)
