"""The reference fixture of the FVA tests (tests/golden/fva_irs.npz, written by tests/golden/gen_fva_golden.py): the controller that
replays it and the bounds it is met at.  The book is tests/xva_cases.py."""
import numpy as np

import cases
import xva_cases as xc
from mcx.metrics.fva_metric import FVAMetric


def golden_controller(backend, metric_cls=FVAMetric):
    """the book of the fixture with the reference's recorded draws injected and its two spread curves -> (controller, fixture)"""
    g = cases.load_golden("fva_irs")
    borrow = dict(zip(g["borrow_tenors"].tolist(), g["borrow_spreads"].tolist()))
    lend = dict(zip(g["lend_tenors"].tolist(), g["lend_spreads"].tolist()))
    sc = xc.controller(backend, [metric_cls(borrow, lend, counterparty_id="cp", own_id="own")], n_main=g["z_main"].shape[1],
                       n_pre=g["z_pre"].shape[1], timeline=g["metric_exposure_timeline"])
    for key, z in (("main", g["z_main"]), ("pre", g["z_pre"])):
        sc._inject[key] = (backend.from_numpy(np.ascontiguousarray(np.transpose(z, (0, 2, 1)))), None)      # [S][n_z][N]
    return sc, g


def assert_meets_golden(sc, res, g):
    """the bounds of xva_cases.assert_meets_golden (tests/test_hip_parity.py): exposures, values, Monte-Carlo errors"""
    ours = xc.values(res, 0, 0)
    assert np.allclose(sc.last_state["expo"][0].cpu().numpy(), g["exposures_0"], rtol=1e-8, atol=1e-10)
    assert ours.shape == g["result_0_0"].shape == (3, 2) and list(g["evaluations"]) == ["fca", "fba", "fva"]
    assert np.all(g["result_0_0"][:2, 0] > 0.0)
    assert np.allclose(ours[:, 0], g["result_0_0"][:, 0], rtol=1e-8, atol=1e-10), (ours[:, 0], g["result_0_0"][:, 0])
    assert np.allclose(ours[:, 1], g["result_0_0"][:, 1], rtol=1e-6, atol=1e-12), (ours[:, 1], g["result_0_0"][:, 1])
