"""DVAMetric / BilateralCVAMetric end to end on the GPU, through run_simulation(): the native route (mcx_reduce_xva, csrc/k4_xva.hip)
against the same controller with non-native subclasses of the two metrics — the host forms of mcx/metrics/bcva_metric.py, pinned
to the numpy restatement in tests/test_xva_host.py — at the bounds tests/test_plugin_metrics.py uses for CVA (1e-12 / 1e-9)."""
import numpy as np
import pytest

import xva_cases as xc
from mcx import _native
from mcx.metrics.bcva_metric import BilateralCVAMetric
from mcx.metrics.cva_metric import CVAMetric
from mcx.metrics.dva_metric import DVAMetric
from mcx.products.swap import IRSType

pytestmark = pytest.mark.gpu


class HostBCVA(BilateralCVAMetric):
    _native = False


class HostDVA(DVAMetric):
    _native = False


def bcva(cls=BilateralCVAMetric):
    return cls("cp", "own", xc.R_CP, xc.R_OWN)


def close(a, b, tag):
    assert np.allclose(a[:, 0], b[:, 0], rtol=1e-12, atol=0.0), (tag, a[:, 0], b[:, 0])
    assert np.allclose(a[:, 1], b[:, 1], rtol=1e-9, atol=0.0), (tag, a[:, 1], b[:, 1])


@pytest.mark.parametrize("kind", ["plain", "collateralised"])
def test_native_route_equals_the_host_forms(kind, hip):
    """one run with both native metrics (they share the own name: atoms do not collide) against one run per host form.
    collateralised: threshold and margin period of risk, the delayed rows of dev_unsec"""
    kw = {} if kind == "plain" else dict(threshold=xc.THRESHOLD, mpor=xc.MPOR)
    sc = xc.controller(hip, [bcva(), DVAMetric("own", xc.R_OWN)], n_main=4099, **kw)
    res = sc.run_simulation()
    assert sc._fused is None and res.metric_names == ["bcva[cp|own]", "dva[own]"]
    sc_h = xc.controller(hip, [bcva(HostBCVA)], n_main=4099, **kw)
    host = xc.values(sc_h.run_simulation())
    assert sc_h._fused is None
    host_dva = xc.values(xc.controller(hip, [HostDVA("own", xc.R_OWN)], n_main=4099, **kw).run_simulation())
    got, dva = xc.values(res, 0, 0), xc.values(res, 0, 1)
    assert got.shape == (5, 2) and np.all(got[:4, 0] > 0.0)
    close(got, host, kind)
    close(dva, host_dva, kind)
    assert tuple(dva[0]) == tuple(got[1])                                  # the same kernel arithmetic, the same reduction


def test_cva_and_bilateral_cva_on_one_counterparty_in_one_run(hip):
    sc = xc.controller(hip, [CVAMetric("cp", xc.R_CP), bcva()], n_main=4099)
    res = sc.run_simulation()
    cva, bil = xc.values(res, 0, 0), xc.values(res, 0, 1)
    assert sc._fused is None and cva[0, 0] > 0.0
    assert np.isclose(cva[0, 0], bil[0, 0], rtol=1e-12, atol=0.0) and np.isclose(cva[0, 1], bil[0, 1], rtol=1e-9, atol=0.0)
    # and the netting set of another counterparty: zeros for both, five of them for the bilateral metric
    res = xc.controller(hip, [CVAMetric("cp", xc.R_CP), bcva()], n_main=256, counterparty_id="someone_else").run_simulation()
    assert [tuple(r) for r in xc.values(res, 0, 0)] == [(0.0, 0.0)] and [tuple(r) for r in xc.values(res, 0, 1)] == [(0.0, 0.0)] * 5


def test_dva_equals_cva_of_the_mirrored_book(hip):
    dva = xc.values(xc.controller(hip, [DVAMetric("own", xc.R_OWN)], n_main=4099, counterparty_id=None).run_simulation())[0]
    sc = xc.controller(hip, [CVAMetric("own", xc.R_OWN)], n_main=4099, counterparty_id=None, irs_type=IRSType.RECEIVER)
    sc.allow_fused = False
    cva = xc.values(sc.run_simulation())[0]
    assert dva[0] > 0.0 and np.isclose(dva[0], cva[0], rtol=1e-12, atol=0.0) and np.isclose(dva[1], cva[1], rtol=1e-9, atol=0.0)


def test_one_exposure_date_gives_exact_zeros(hip):
    res = xc.controller(hip, [bcva(), DVAMetric("own", xc.R_OWN)], n_main=300, timeline=np.array([0.5])).run_simulation()
    assert [tuple(r) for r in xc.values(res, 0, 0)] == [(0.0, 0.0)] * 5 and tuple(xc.values(res, 0, 1)[0]) == (0.0, 0.0)


def test_native_route_meets_the_reference_fixture(hip):
    """tests/golden/xva_irs.npz: the reference engine with a CVAMetric subclass that evaluates the table, on recorded draws; with
    CVAMetric beside it, whose value must be the fixture's cva too"""
    sc, g = xc.golden_controller(hip, [bcva(), CVAMetric("cp", xc.R_CP)])
    res = sc.run_simulation()
    assert sc._fused is None
    xc.assert_meets_golden(sc, res, g)
    cva = xc.values(res, 0, 1)[0]
    assert np.isclose(cva[0], g["result_0_0"][0, 0], rtol=1e-8, atol=1e-10) and np.isclose(cva[1], g["result_0_0"][0, 1], rtol=1e-6, atol=1e-12)


def test_three_emulated_ranks_reproduce_one_shard(hip):
    """values at the issue's rtol 1e-9; the Monte-Carlo errors at 1e-6, the convention of tests/test_emulated_ranks.py: the ranks'
    records are merged by Chan's update, whose M2 carries the rounding of the between-rank term"""
    from emulated_ranks import run_ranks
    n_main, n_pre = 3001, 1000

    def build(be):
        sc = xc.controller(be, [bcva(), DVAMetric("own", xc.R_OWN)], n_main=n_main, n_pre=n_pre, threshold=xc.THRESHOLD, mpor=xc.MPOR)
        sc.materialize = False
        return sc

    ref = build(hip).run_simulation()
    out, calls = run_ranks(3, lambda rank: build(_native.HipBackend(0)), lambda sc, rank: sc.run_simulation())
    assert calls["all_gather"] > 0
    for rank, got in enumerate(out):
        for m_i in range(2):
            a, b = xc.values(ref, 0, m_i), xc.values(got, 0, m_i)
            assert np.allclose(a[:, 0], b[:, 0], rtol=1e-9, atol=0.0), (rank, m_i, a[:, 0], b[:, 0])
            assert np.allclose(a[:, 1], b[:, 1], rtol=1e-6, atol=0.0), (rank, m_i, a[:, 1], b[:, 1])


def test_differentiate_takes_the_bump_route_and_mirrors_the_cva_gradient(hip):
    """no forward-mode dual of k4_xva: the book is bumped.  The DVA gradient of the payer book equals the CVA gradient of the
    receiver book, both bumped (forward_mode off for the latter), at rtol 1e-9; the entries of the counterparty's parameters are
    exactly zero on both sides (neither metric reads that factor)"""
    sc = xc.controller(hip, [DVAMetric("own", xc.R_OWN)], n_main=512, n_pre=512, counterparty_id=None, differentiate=True)
    res = sc.run_simulation()
    P = len(sc.model.get_model_params())
    assert sc.timings["tangent"] is False and sc.timings["bumped_passes"] == 2 * P
    g = np.array(res.derivatives[0][0], dtype=np.float64)[0]
    sc_m = xc.controller(hip, [CVAMetric("own", xc.R_OWN)], n_main=512, n_pre=512, counterparty_id=None, irs_type=IRSType.RECEIVER,
                         differentiate=True)
    sc_m.forward_mode = False
    res_m = sc_m.run_simulation()
    assert sc_m.timings["tangent"] is False and sc_m.timings["bumped_passes"] == 2 * P
    g_m = np.array(res_m.derivatives[0][0], dtype=np.float64)[0]
    print("dva gradient", g, "mirrored cva gradient", g_m, "largest difference", np.abs(g - g_m).max())
    assert np.isfinite(g).all() and np.abs(g).max() > 0.0
    assert np.allclose(g, g_m, rtol=1e-9, atol=0.0)
