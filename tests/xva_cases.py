"""The books of the bilateral-xVA tests: one interest-rate swap under ModelConfig[Vasicek, CIR++(cp), CIR++(own)] with non-zero
correlations between all three factors.  The short rate starts at its mean and the swap pays (or receives) that rate, so the
exposure takes both signs on every date after the first."""
import numpy as np

import cases
from mcx.controller.controller import SimulationController
from mcx.metrics.risk_metrics import RiskMetrics
from mcx.models.cirpp import CIRPPModel
from mcx.models.model_config import ModelConfig
from mcx.models.vasicek import VasicekModel
from mcx.products.netting_set import NettingSet
from mcx.products.swap import InterestRateSwap, IRSType

OWN_HAZARDS = {t: 0.6 * h + 0.004 for t, h in cases.HAZARDS.items()}
R_CP, R_OWN = 0.4, 0.35
TIMELINE = np.arange(11) * 0.25
THRESHOLD, MPOR = 0.002, 0.25


def models(own=True):
    ir = VasicekModel(0.0, 0.03, 0.03, 0.1, 0.01, asset_id="irs")
    cp = CIRPPModel(0.0, "cp", cases.HAZARDS, kappa=0.1, theta=0.01, volatility=0.02, y0=1e-4)
    if not own:
        return ModelConfig([ir, cp], inter_asset_correlation_matrix=np.array([0.4]))
    me = CIRPPModel(0.0, "own", OWN_HAZARDS, kappa=0.2, theta=0.015, volatility=0.03, y0=2e-4)
    # blocks over the model pairs (irs, cp), (irs, own), (cp, own)
    return ModelConfig([ir, cp, me], inter_asset_correlation_matrix=[np.array([0.4]), np.array([-0.3]), np.array([0.25])])


def netting_sets(irs_type=IRSType.PAYER, counterparty_id="cp", threshold=0.0, mpor=None):
    irs = InterestRateSwap(0.0, 2.5, 1.0, 0.03, 0.25, 0.25, irs_type, "irs")
    return [NettingSet(name="swap", products=[irs], counterparty_id=counterparty_id, threshold=threshold, margin_period_of_risk=mpor)]


def controller(backend, metrics, n_main=1024, n_pre=1024, timeline=TIMELINE, differentiate=False, model=None, **ns_kw):
    rm = RiskMetrics(metrics, exposure_timeline=timeline)
    sc = SimulationController(netting_sets(**ns_kw), models() if model is None else model, rm, n_main, n_pre, 2, cases.E,
                              differentiate=differentiate, backend=backend)
    sc.materialize = True
    return sc


def golden_controller(backend, metrics):
    """the book of tests/golden/gen_xva_golden.py with the reference's recorded draws injected -> (controller, fixture)"""
    g = cases.load_golden("xva_irs")
    n = g["z_main"].shape[1]
    sc = controller(backend, metrics, n_main=n, n_pre=g["z_pre"].shape[1], timeline=g["metric_exposure_timeline"])
    for key, z in (("main", g["z_main"]), ("pre", g["z_pre"])):
        sc._inject[key] = (backend.from_numpy(np.ascontiguousarray(np.transpose(z, (0, 2, 1)))), None)      # [S][n_z][N]
    return sc, g


def assert_meets_golden(sc, res, g, m_i=0):
    """the bounds tests/test_hip_parity.py uses for exposures, CVA values and Monte-Carlo errors against the reference"""
    ours = values(res, 0, m_i)
    assert np.allclose(sc.last_state["expo"][0].cpu().numpy(), g["exposures_0"], rtol=1e-8, atol=1e-10)
    assert ours.shape == g["result_0_0"].shape == (5, 2) and list(g["evaluations"]) == ["cva", "dva", "cva_ftd", "dva_ftd", "bcva"]
    assert np.allclose(ours[:, 0], g["result_0_0"][:, 0], rtol=1e-8, atol=1e-10), (ours[:, 0], g["result_0_0"][:, 0])
    assert np.allclose(ours[:, 1], g["result_0_0"][:, 1], rtol=1e-6, atol=1e-12), (ours[:, 1], g["result_0_0"][:, 1])


def values(res, ns_i=0, m_i=0):
    """[evaluations][2] (value, error) of one metric of one netting set"""
    return np.array(res.results[ns_i][m_i], dtype=np.float64)
