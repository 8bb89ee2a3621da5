"""Gas-storage controller cases, written once for two class families: tests/golden/gen_storage_golden.py builds them with the
reference's classes, the tests with mcx's (`mod` = dict of classes, as `_mixed_book_products` of gen_golden.py does).  This file
imports neither: `mcx_classes()` does it lazily for the tests.

name -> (builder, n_pre, n_main, num_steps, scheme name, regression degree)"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HAZARDS = {0.5: 0.0064, 1.0: 0.0155, 2.0: 0.0097, 3.0: 0.0156, 5.0: 0.0228, 10.0: 0.0061}
CLASS_NAMES = ("Storage", "StorageConfig", "NettingSet", "RiskMetrics", "PVMetric", "EPEMetric", "ENEMetric", "PFEMetric", "CVAMetric",
               "SchwartzTwoFactorModel", "BlackScholesMulti", "CIRPPModel", "ModelConfig", "EuropeanOption", "Equity", "OptionType")


def mcx_classes():
    from mcx.metrics.cva_metric import CVAMetric
    from mcx.metrics.ene_metric import ENEMetric
    from mcx.metrics.epe_metric import EPEMetric
    from mcx.metrics.pfe_metric import PFEMetric
    from mcx.metrics.pv_metric import PVMetric
    from mcx.metrics.risk_metrics import RiskMetrics
    from mcx.models.black_scholes_multi import BlackScholesMulti
    from mcx.models.cirpp import CIRPPModel
    from mcx.models.model_config import ModelConfig
    from mcx.models.schwartz_two_factor import SchwartzTwoFactorModel
    from mcx.products.equity import Equity
    from mcx.products.european_option import EuropeanOption
    from mcx.products.netting_set import NettingSet
    from mcx.products.product import OptionType
    from mcx.products.storage import Storage
    from mcx.products.storage_helpers import StorageConfig
    loc = locals()
    return {k: loc[k] for k in CLASS_NAMES}


def _gas_model(mod):
    return mod["SchwartzTwoFactorModel"](0.0, [0.0, 2.0, 5.0, 8.0], [30.0, 32.0, 29.0, 31.0], rate=0.002, short_term_mean_reversion=0.3,
                                         short_term_vol=0.12, long_term_drift=0.001, long_term_vol=0.04, rho=0.3, asset_id="gas")


def _daily_store(mod, S, end, windows, rollout=1.0, initial=4.0):
    """3-knot injection / 2-knot withdrawal curves, an injection-cost step at day 4"""
    c = mod["StorageConfig"]()
    for w in windows:
        c.add_volume_constraint(*w, 0.0)
    for p, r in ((0.0, 3.0), (6.0, 1.5), (10.0, 0.5)):
        c.add_injection_flexibility(0.0, end + 1, p, r)
    for p, r in ((0.0, 1.0), (6.0, 2.5)):
        c.add_withdrawal_flexibility(0.0, end + 1, p, r)
    c.add_variable_injection_cost(0.0, 0.2)
    c.add_variable_injection_cost(4.0, 0.3)
    c.add_variable_withdrawal_cost(0.0, 0.1)
    return mod["Storage"]("gas", 0.0, float(end), initial, c, S, rollout)


def _profile_metrics(mod, timeline):
    return mod["RiskMetrics"]([mod["PVMetric"](), mod["EPEMetric"](), mod["ENEMetric"](), mod["PFEMetric"](0.9)],
                              exposure_timeline=np.array(timeline))


def storage_const(mod):
    """one window [0, 12]; a non-action exposure date (2.5) and the end date (exposure 0)"""
    p = _daily_store(mod, 5, 8.0, [(0.0, 9.0, 0.0, 12.0)])
    return [mod["NettingSet"](name="st", products=[p])], _gas_model(mod), _profile_metrics(mod, [0.0, 1.0, 2.5, 4.0, 6.0, 8.0])


def storage_shift(mod):
    """S = 10 > MCX_MAX_STATES; windows [0,12] -> [2,10] -> [0,6]: the optimiser's backward bisection and restart run"""
    p = _daily_store(mod, 10, 8.0, [(0.0, 3.0, 0.0, 12.0), (3.0, 5.0, 2.0, 10.0), (5.0, 9.0, 0.0, 6.0)])
    return [mod["NettingSet"](name="st", products=[p])], _gas_model(mod), _profile_metrics(mod, [0.0, 1.0, 2.5, 4.0, 6.0, 8.0])


def storage_short_last(mod):
    """end date 7.5 with a rollout interval of 2: action dates 0, 2, 4, 6, the last period 1.5 long"""
    p = _daily_store(mod, 6, 7.5, [(0.0, 8.5, 0.0, 12.0)], rollout=2.0, initial=5.0)
    return [mod["NettingSet"](name="st", products=[p])], _gas_model(mod), _profile_metrics(mod, [0.0, 2.0, 3.0, 6.0, 7.5])


def _equity_store(mod, asset, S, start, end, dt, cap, init, c_inj, c_wd):
    c = mod["StorageConfig"]()
    c.add_volume_constraint(start, end + 1, 0.0, cap, 0.0)
    c.add_injection_flexibility(start, end + 1, 0.0, 0.15 * cap / dt)
    c.add_injection_flexibility(start, end + 1, 0.6 * cap, 0.05 * cap / dt)
    c.add_withdrawal_flexibility(start, end + 1, 0.0, 0.05 * cap / dt)
    c.add_withdrawal_flexibility(start, end + 1, 0.6 * cap, 0.15 * cap / dt)
    c.add_variable_injection_cost(start, c_inj)
    c.add_variable_withdrawal_cost(start, c_wd)
    return mod["Storage"](asset, start, end, init, c, S, rollout_interval=dt)


def storage_mixed(mod):
    """BlackScholesMulti(2) + CIR++: a storage and a European call share a collateralised netting set (threshold, margin period),
    a second netting set holds a storage that starts after the calibration date; CVA + EPE + PV"""
    corr = np.array([[1.0, 0.35], [0.35, 1.0]])
    market = mod["BlackScholesMulti"](0.0, 0.03, ["a1", "a2"], [100.0, 40.0], [0.2, 0.35], corr)
    credit = mod["CIRPPModel"](0.0, "cp", dict(HAZARDS), kappa=0.1, theta=0.01, volatility=0.02, y0=1e-4)
    model = mod["ModelConfig"]([market, credit], inter_asset_correlation_matrix=[np.full((2, 1), 0.2)])
    s1 = _equity_store(mod, "a2", 7, 0.0, 1.0, 0.125, 10.0, 2.0, -1.0, 0.3)      # (an injection rebate: a martingale spot alone never injects)
    s1.name = "store1"
    call = mod["EuropeanOption"](mod["Equity"]("a1"), 1.0, 100.0, mod["OptionType"].CALL, asset_id="a1")
    s2 = _equity_store(mod, "a1", 4, 0.25, 1.0, 0.25, 5.0, 1.0, 0.5, 0.3)
    s2.name = "store2"
    ns = [mod["NettingSet"](name="mix", products=[s1, call], counterparty_id="cp", threshold=0.5, margin_period_of_risk=0.125),
          mod["NettingSet"](name="solo", products=[s2], counterparty_id="cp")]
    rm = mod["RiskMetrics"]([mod["CVAMetric"]("cp", 0.4), mod["EPEMetric"](), mod["PVMetric"]()], exposure_timeline=np.linspace(0.0, 1.0, 9))
    return ns, model, rm


CASES = {
    "storage_const": (storage_const, 1024, 1024, 2, "ANALYTICAL", 2),
    "storage_shift": (storage_shift, 1024, 1024, 2, "ANALYTICAL", 3),
    "storage_short_last": (storage_short_last, 1024, 1024, 3, "EULER", 2),
    "storage_mixed": (storage_mixed, 1024, 1024, 1, "EULER", 2),
}


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def make_controller(name, backend, inject=True, **overrides):
    """the mcx controller of a case (materialised plan), with the fixture's draws injected"""
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    from mcx.maths.regression import PolyomialRegression
    build, n_pre, n_main, steps, scheme, degree = CASES[name]
    ns, model, rm = build(mcx_classes())
    sc = SimulationController(ns, model, rm, overrides.get("n_main", n_main), overrides.get("n_pre", n_pre), steps,
                              getattr(SimulationScheme, scheme), False, regression_function=PolyomialRegression(degree=degree), backend=backend)
    sc.materialize = True
    g = load_golden(name) if inject else None
    if inject:
        for phase in ("pre", "main"):
            z = backend.from_numpy(np.ascontiguousarray(np.transpose(g["z_" + phase], (0, 2, 1))))      # [steps][n_z][N]
            sc._inject[phase] = (z, None)
    return sc, g


# ---- the reference's own scenarios (tests/storage_s2f_cases.py, test_storage.py:116-159), rebuilt from storage_anchors.npz ------
def anchor_scenario(g, name, mod):
    """(storage, model) of scenario `name` from the arrays the generator recorded"""
    c = mod["StorageConfig"]()
    for w in g[name + "_windows"]:
        c.add_volume_constraint(float(w[0]), float(w[1]), float(w[2]), float(w[3]), 0.0)
    for r in g[name + "_injection"]:
        c.add_injection_flexibility(float(r[0]), float(r[1]), float(r[2]), float(r[3]))
    for r in g[name + "_withdrawal"]:
        c.add_withdrawal_flexibility(float(r[0]), float(r[1]), float(r[2]), float(r[3]))
    end, initial, c_inj, c_wd, S, rollout = (float(v) for v in g[name + "_scalars"])
    c.add_variable_injection_cost(0.0, c_inj)
    c.add_variable_withdrawal_cost(0.0, c_wd)
    p = mod["Storage"]("thegasprice", 0.0, end, initial, c, int(S), rollout)
    rate, kappa, sig_s, mu, sig_l, rho = (float(v) for v in g[name + "_model"])
    model = mod["SchwartzTwoFactorModel"](0.0, [float(t) for t in g[name + "_curve_t"]], [float(v) for v in g[name + "_curve_v"]],
                                          rate=rate, short_term_mean_reversion=kappa, short_term_vol=sig_s, long_term_drift=mu,
                                          long_term_vol=sig_l, rho=rho, asset_id="thegasprice")
    return p, model
