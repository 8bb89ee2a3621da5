"""FVAMetric end to end on the GPU, through run_simulation(): the native route (mcx_reduce_fva, csrc/k4_fva.hip) against the same
controller with a non-native subclass of the metric — the host form of mcx/metrics/fva_metric.py, pinned to the numpy restatement in
tests/test_fva_host.py — at 1e-12 / 1e-9; beside the other xVA metrics, on collateralised and gated sets, under a single model, on
emulated ranks, mirrored, differentiated, and against the reference fixture.  1,024 + 1,024 paths unless said."""
import numpy as np
import pytest

import cases
import fva_cases as fc
import fva_reference as fr
import xva_cases as xc
from mcx import _native
from mcx.controller.controller import SimulationController
from mcx.metrics.bcva_metric import BilateralCVAMetric
from mcx.metrics.cva_metric import CVAMetric
from mcx.metrics.fva_metric import FVAMetric, funding_weights
from mcx.metrics.risk_metrics import RiskMetrics
from mcx.models.vasicek import VasicekModel
from mcx.products.netting_set import NettingSet
from mcx.products.swap import InterestRateSwap, IRSType

pytestmark = pytest.mark.gpu


class HostFVA(FVAMetric):
    _native = False


def fva(cls=FVAMetric, cp="cp", own="own", borrow=fr.BORROW_CURVE, lend=fr.LEND_CURVE):
    return cls(borrow, lend, counterparty_id=cp, own_id=own)


def close(a, b, tag):
    assert np.allclose(a[:, 0], b[:, 0], rtol=1e-12, atol=0.0), (tag, a[:, 0], b[:, 0])
    assert np.allclose(a[:, 1], b[:, 1], rtol=1e-9, atol=0.0), (tag, a[:, 1], b[:, 1])


@pytest.mark.parametrize("names", [("cp", "own"), (None, "own"), ("cp", None), (None, None)], ids=["both", "own", "cp", "none"])
@pytest.mark.parametrize("kind", ["plain", "collateralised"])
def test_native_route_equals_the_host_form(kind, names, hip):
    """collateralised: threshold and margin period of risk, the delayed rows of dev_unsec"""
    kw = {} if kind == "plain" else dict(threshold=xc.THRESHOLD, mpor=xc.MPOR)
    sc = xc.controller(hip, [fva(FVAMetric, *names)], **kw)
    got = xc.values(sc.run_simulation())
    sc_h = xc.controller(hip, [fva(HostFVA, *names)], **kw)
    host = xc.values(sc_h.run_simulation())
    assert sc._fused is None and sc_h._fused is None
    assert got.shape == (3, 2) and np.all(got[:2, 0] > 0.0)
    close(got, host, (kind, names))


def test_fva_beside_the_other_xva_metrics_in_one_run(hip):
    """FVA, bilateral CVA and CVA share the two names in one RiskMetrics: atoms do not collide.  Every metric keeps the value it has
    in a run of its own"""
    metrics = [fva(), BilateralCVAMetric("cp", "own", xc.R_CP, xc.R_OWN), CVAMetric("cp", xc.R_CP), cases.EPEMetric()]
    sc = xc.controller(hip, metrics)
    res = sc.run_simulation()
    assert sc._fused is None and res.metric_names == ["fva[cp|own]", "bcva[cp|own]", "cva[cp]", "epe"]
    alone = xc.values(xc.controller(hip, [fva()]).run_simulation())
    close(xc.values(res, 0, 0), alone, "fva")
    bil = xc.values(xc.controller(hip, [BilateralCVAMetric("cp", "own", xc.R_CP, xc.R_OWN)]).run_simulation())
    close(xc.values(res, 0, 1), bil, "bcva")
    cva = xc.values(res, 0, 2)
    assert np.isclose(cva[0, 0], bil[0, 0], rtol=1e-12, atol=0.0) and len(res.results[0][3]) == len(xc.TIMELINE)


def test_second_netting_set_of_another_counterparty(hip):
    """exact-zero rows for the metric that names `cp` on the set of `other`; a metric without a counterparty applies to both sets"""
    def swap(kind):
        return InterestRateSwap(0.0, 2.5, 1.0, 0.03, 0.25, 0.25, kind, "irs")
    sets = [NettingSet(name="a", products=[swap(IRSType.PAYER)], counterparty_id="cp"),
            NettingSet(name="b", products=[swap(IRSType.RECEIVER)], counterparty_id="other", threshold=xc.THRESHOLD)]
    rm = RiskMetrics([fva(), fva(FVAMetric, None, "own"), fva(FVAMetric, None, None)], exposure_timeline=xc.TIMELINE)
    sc = SimulationController(sets, xc.models(), rm, 1024, 1024, 2, cases.E, backend=hip)
    res = sc.run_simulation()
    assert sc._fused is None
    assert [tuple(r) for r in xc.values(res, 1, 0)] == [(0.0, 0.0)] * 3
    for ns_i, m_i in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2)):
        v = xc.values(res, ns_i, m_i)
        assert v.shape == (3, 2) and np.all(v[:2, 0] > 0.0) and np.all(v[:, 1] > 0.0), (ns_i, m_i, v)
    # a survival probability only shrinks a leg
    for ns_i in (0, 1):
        assert np.all(xc.values(res, ns_i, 1)[:2, 0] < xc.values(res, ns_i, 2)[:2, 0])


def test_unnamed_metric_under_a_single_vasicek_model(hip):
    model = VasicekModel(0.0, 0.03, 0.03, 0.1, 0.01, asset_id="irs")
    sc = xc.controller(hip, [fva(FVAMetric, None, None), cases.EPEMetric(), cases.ENEMetric()], model=model)
    res = sc.run_simulation()
    got = xc.values(res, 0, 0)
    epe, ene = xc.values(res, 0, 1)[:, 0], xc.values(res, 0, 2)[:, 0]
    wb, wl = np.array(funding_weights(fr.BORROW_CURVE, xc.TIMELINE)), np.array(funding_weights(fr.LEND_CURVE, xc.TIMELINE))
    assert sc._fused is None and got[0, 0] > 0.0 and got[1, 0] > 0.0
    assert np.isclose(got[0, 0], float(np.dot(epe[:-1], wb)), rtol=1e-12, atol=0.0)
    assert np.isclose(got[1, 0], -float(np.dot(ene[:-1], wl)), rtol=1e-12, atol=0.0)
    host = xc.values(xc.controller(hip, [fva(HostFVA, None, None)], model=model).run_simulation())
    close(got, host, "vasicek")


def test_one_exposure_date_gives_exact_zeros(hip):
    res = xc.controller(hip, [fva(), fva(FVAMetric, None, None)], n_main=300, timeline=np.array([0.5])).run_simulation()
    assert [tuple(r) for r in xc.values(res, 0, 0)] == [(0.0, 0.0)] * 3 == [tuple(r) for r in xc.values(res, 0, 1)]


def test_three_emulated_ranks_reproduce_one_shard(hip):
    """values and Monte-Carlo errors at rtol 1e-9 (the test prints the gaps before it asserts)"""
    from emulated_ranks import run_ranks
    n_main, n_pre = 1024, 1024

    def build(be):
        sc = xc.controller(be, [fva(), fva(FVAMetric, None, None)], n_main=n_main, n_pre=n_pre, threshold=xc.THRESHOLD, mpor=xc.MPOR)
        sc.materialize = False
        return sc

    ref = build(hip).run_simulation()
    out, calls = run_ranks(3, lambda rank: build(_native.HipBackend(0)), lambda sc, rank: sc.run_simulation())
    assert calls["all_gather"] > 0
    for rank, got in enumerate(out):
        for m_i in range(2):
            a, b = xc.values(ref, 0, m_i), xc.values(got, 0, m_i)
            print(f"rank {rank} metric {m_i}: value gap {np.abs(a[:, 0] / b[:, 0] - 1).max():.3e}, error gap {np.abs(a[:, 1] / b[:, 1] - 1).max():.3e}")
            assert np.allclose(a[:, 0], b[:, 0], rtol=1e-9, atol=0.0), (rank, m_i, a[:, 0], b[:, 0])
            assert np.allclose(a[:, 1], b[:, 1], rtol=1e-9, atol=0.0), (rank, m_i, a[:, 1], b[:, 1])


def test_mirrored_book_exchanges_the_legs(hip):
    """the receiver swap with the two spread curves swapped: relu(-x) of one book is relu(x) of the other, same Philox draws"""
    a = xc.values(xc.controller(hip, [fva()]).run_simulation())
    b = xc.values(xc.controller(hip, [fva(borrow=fr.LEND_CURVE, lend=fr.BORROW_CURVE)], irs_type=IRSType.RECEIVER).run_simulation())
    assert a[0, 0] > 0.0 and a[1, 0] > 0.0
    assert np.allclose(a[0], b[1], rtol=1e-12, atol=0.0) and np.allclose(a[1], b[0], rtol=1e-12, atol=0.0)
    assert np.isclose(a[2, 0], -b[2, 0], rtol=1e-12, atol=0.0)


def test_native_route_meets_the_reference_fixture(hip):
    """tests/golden/fva_irs.npz: the reference engine with a CVAMetric subclass that evaluates the table, on recorded draws"""
    sc, g = fc.golden_controller(hip)
    res = sc.run_simulation()
    assert sc._fused is None and res.metric_names == ["fva[cp|own]"]
    fc.assert_meets_golden(sc, res, g)


@pytest.mark.parametrize("tangent_xva", [False, True])
def test_differentiate_bumps_and_sums_the_epe_gradients(tangent_xva, hip):
    """no forward-mode dual of k4_fva: the book is bumped, with or without tangent_xva.  With no names and a flat spread on the
    equally spaced timeline every borrowing weight is the same c, so d fca = c * sum_{k<E-1} d EPE_k of the EPEMetric in the same run:
    both sides are differences of the same bumped runs, only the summation order separates them — 1e-10 of the row's largest entry"""
    s = 0.0125
    sc = xc.controller(hip, [FVAMetric(s), cases.EPEMetric()], differentiate=True)
    sc.tangent_xva = tangent_xva
    res = sc.run_simulation()
    P = len(sc.model.get_model_params())
    assert sc.timings["tangent"] is False and sc.timings["bumped_passes"] == 2 * P
    w = funding_weights(s, xc.TIMELINE)
    assert len(set(w)) == 1 and w[0] > 0.0
    g = np.array(res.derivatives[0][0], dtype=np.float64)
    g_epe = np.array(res.derivatives[0][1], dtype=np.float64)
    assert g.shape == (3, P) and g_epe.shape == (len(xc.TIMELINE), P)
    want = w[0] * g_epe[:-1].sum(axis=0)
    scale = float(np.abs(g[0]).max())
    gap = float(np.abs(g[0] - want).max())
    print(f"tangent_xva={tangent_xva}: d fca {g[0]}, c * sum d EPE {want}, largest gap {gap:.3e} = {gap / scale:.3e} of the largest entry")
    assert scale > 0.0 and np.isfinite(g).all()
    assert gap <= 1e-10 * scale
