"""The cva-date kernel of the one-launch pass (kf_lean.hip lean_date_cva, picked by mcx_fused_create for Vasicek + CIR++ CVA
books whose every date is the merged CVA increment): config-3-shaped books against the CPU oracle on identical Philox counters,
and books that must NOT take it (an added EPE, an exposure output, a Bermudan) against the oracle
through the general date program.  Tolerances are those of the fused CVA tests in test_hip_parity.py."""
import numpy as np
import pytest

import cases
from mcx import _abi

pytestmark = pytest.mark.gpu

HAZARDS = {0.5: 0.0064, 1.0: 0.0155, 2.0: 0.0097, 3.0: 0.0156, 5.0: 0.0228, 10.0: 0.0061, 20.0: 0.0038}


def _irs_book(mat, payer, tenor, hazard_scale, epe=False, bermudan=False):
    from mcx.products.swap import InterestRateSwap, IRSType
    ir = cases.VasicekModel(0.0, rate=0.03, mean=0.05, mean_reversion_speed=0.1, volatility=0.01, asset_id="irs")
    cr = cases.CIRPPModel(0.0, "cp", {t: h * hazard_scale for t, h in HAZARDS.items()}, kappa=0.1, theta=0.01, volatility=0.02, y0=1e-4)
    model = cases.ModelConfig([ir, cr], inter_asset_correlation_matrix=np.array([0.5]))
    swap = InterestRateSwap(0.0, mat, 1.0, 0.03, tenor, tenor, IRSType.PAYER if payer else IRSType.RECEIVER, "irs")
    prod = swap
    if bermudan:
        n_ex = 4
        prod = cases.BermudanOption(swap, [mat * (k + 1) / (n_ex + 1) for k in range(n_ex)], 0.0, cases.OptionType.CALL, asset_id="irs")
    ns = [cases.NettingSet(name="irs", products=[prod], counterparty_id="cp")]
    mets = [cases.CVAMetric("cp", 0.4)] + ([cases.EPEMetric()] if epe else [])
    return ns, model, cases.RiskMetrics(mets, exposure_timeline=np.arange(0.0, mat + 1e-9, 0.25))


def _run(build, n_main, steps, hip, oracle, materialize=False):
    out = {}
    for be in (hip, oracle):
        ns, model, rm = build()
        sc = cases.SimulationController(ns, model, rm, n_main, 4096, steps, cases.E, backend=be)
        if be is hip:
            sc.main_plan = "fused"
            sc.materialize = materialize
        out[be.name] = sc.run_simulation().results
        if be is hip:      # the route of the pass just run (mcx_fused_describe: the host function that chose the launch)
            out["route"] = hip.fused_describe(sc._fused, False, True)
            out["expo"] = sc.last_state["expo"]
    return out


def _check(out, tag):
    for ns_i in range(len(out["hip"])):
        for m_i in range(len(out["hip"][ns_i])):
            a, b = np.array(out["hip"][ns_i][m_i], dtype=np.float64), np.array(out["oracle"][ns_i][m_i], dtype=np.float64)
            assert np.allclose(a[:, 0], b[:, 0], rtol=1e-8, atol=1e-10), (tag, ns_i, m_i, a[:, 0], b[:, 0])
            assert np.allclose(a[:, 1], b[:, 1], rtol=1e-5, atol=1e-11), (tag, ns_i, m_i, a[:, 1], b[:, 1])


# (maturity, payer, tenor, hazard scale, paths, sub-steps): ragged path counts on both launch shapes (one path per lane below
# 2 x CUs block-tiles, two from there on)
BOOKS = [(12.5, True, 0.25, 1.0, 5000, 5), (3.0, False, 0.5, 2.0, 70001, 3), (5.0, True, 0.25, 0.5, 1 << 18, 2),
         (2.0, False, 0.25, 3.0, 300001, 4)]


@pytest.mark.parametrize("book", BOOKS, ids=[f"mat{b[0]}-{'payer' if b[1] else 'receiver'}-n{b[4]}" for b in BOOKS])
def test_cva_books_on_the_cva_date_kernel(book, hip, oracle):
    mat, payer, tenor, hz, n, steps = book
    _check(_run(lambda: _irs_book(mat, payer, tenor, hz), n, steps, hip, oracle), book)


NOT_QUALIFYING = {
    "added_epe": dict(epe=True),
    "bermudan": dict(bermudan=True),
}


@pytest.mark.parametrize("kind", list(NOT_QUALIFYING))
def test_books_off_the_cva_date_kernel(kind, hip, oracle):
    kw = NOT_QUALIFYING[kind]
    out = _run(lambda: _irs_book(3.0, True, 0.25, 1.0, **kw), 300001, 2, hip, oracle)
    d = out["route"]
    # every date straight-line: kf_lean's general date program, not the cva-date kernel and not the interpreter
    assert d["kernel"] == "lean" and d["lean"] and (d["valid"] == 1).all() and not d["cva_dates"], d
    assert (d["flags"] & (_abi.FD_PROFILE if kind == "added_epe" else _abi.FD_EXERCISE)).any(), d
    _check(out, kind)


def test_exposure_output_runs_the_general_program(hip, oracle):
    """materialize: the pass also writes paths and exposures, which only the general date program does"""
    out = _run(lambda: _irs_book(3.0, True, 0.25, 1.0), 300001, 2, hip, oracle, materialize=True)
    d = out["route"]
    # the book has the cva-date records, but a run with outputs launches kf_lean's general program (fused_run_impl: a.cva_dates)
    assert d["kernel"] == "lean" and (d["valid"] == 1).all() and d["cva_dates"] and out["expo"] is not None, d
    _check(out, "materialize")
