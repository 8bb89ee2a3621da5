"""The host-side seams of the forward-mode book pass (mcx/aad.py run_with_tangent_book; DESIGN.md "Forward-mode book pass: the stages
of the driver"), without a GPU: the shared regression helpers, the descriptor tangents in both modes, the slot table of the analytic
Black-Scholes exposure events, the metric scatter on synthetic images and the order of the gates.  The stages that launch kernels run
end to end in the *_gpu.py tests of the tangent pass."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import cases
import large_cva_cases
from mcx import _abi, aad
from mcx.maths.regression import regression_centering

NP = _abi.TANGENT_NP


@pytest.fixture(scope="module")
def mixed(oracle):
    """the compiled mixed_cva controller (Black-Scholes + Vasicek + CIR++) at 64 paths"""
    ns, model, rm = cases.mixed_cva()
    sc = cases.SimulationController(ns, model, rm, 64, 64, 2, cases.E, backend=oracle)
    sc.run_simulation()
    return sc


# ---- centering and plan ----------------------------------------------------------------------------------------------------------------
def test_centering_is_the_literal_formula():
    x_range = {7: (-0.75, 2.5), 9: (1.5, 1.5)}
    assert regression_centering(x_range, 7) == (0.5 * (-0.75 + 2.5), 2.0 / (2.5 - -0.75), False)
    assert regression_centering(x_range, 9) == (1.5, 1.0, True)
    assert regression_centering({0: (float("nan"), 1.0)}, 0)[2] is True       # not (max > min): an unordered range is degenerate


def test_regression_plan_is_the_list_the_driver_built(mixed):
    sc = mixed
    jobs = [(p_i, p) for p_i, p in enumerate(sc.products) if p_i in sc._mc_set and sc._product_requires_regression(p)]
    want = [(p_i, p, sc._regression_schedule(p_i, p)) for p_i, p in jobs]
    want = [(p_i, p, sched, sc._regression_atoms(sched, p.asset_ids[0])) for p_i, p, sched in want]
    got, storages = sc._regression_plan()
    assert storages == [] and len(got) == 4 and [j[0] for j in got] == [0, 1, 2, 3]
    assert got == want


# ---- descriptor tangents ---------------------------------------------------------------------------------------------------------------
def _gap(d4, dc):
    """largest difference of two derivative blocks [...][P] relative to the largest entry of the block's column of that parameter"""
    worst = 0.0
    for j in range(dc.shape[-1]):
        big = np.abs(dc[..., j]).max() if dc[..., j].size else 0.0
        if big == 0.0:                                                        # the block does not depend on theta_j: equal evaluations
            assert not d4[..., j].any()
            continue
        worst = max(worst, float(np.abs(d4[..., j] - dc[..., j]).max() / big))
    return worst


def test_descriptor_tangents_in_both_modes(mixed, monkeypatch):
    """complex step is exact to rounding and the reference here; the 4-point formula with h = 1e-3 |theta| has truncation O(h^4) and
    rounding eps |f| / h.  Largest gap measured over all blocks and the 11 parameters of mixed_cva, relative to the largest entry of
    the parameter's column: 1.45e-10, in the atoms block for the Vasicek volatility (theta = 0.01, h = 1e-5: an exponent coefficient
    of value 8.6e-4 whose derivative is 4.3e-5, so the rounding term eps |f| / (h |f'|) is ~4e-10 there); every other column stays
    below 1.6e-12, slots and init below 1e-13.  Asserted at the measured gap plus one decimal order."""
    monkeypatch.setenv("MCX_DESCRIPTOR_FD", "2")                              # an explicit mode wins over the environment
    model = mixed.model
    P = len(model.get_model_params())
    assert P == 11 and P > 2 * NP
    d0, dc = aad.descriptor_tangents(mixed, model, False, mode="complex")
    d0_4, d4 = aad.descriptor_tangents(mixed, model, False, mode="4")
    assert set(dc) == set(d0) == set(d4) == {"slots", "init", "aux", "atoms"}
    worst = {}
    for k in d0:
        assert np.array_equal(d0[k], d0_4[k]) and dc[k].shape == d4[k].shape == d0[k].shape + (P,)
        assert np.abs(dc[k]).max() > 0.0 or k == "aux"                        # (EULER: these models have no per-step constants)
        worst[k] = _gap(d4[k], dc[k])
    print("4-point against complex step, largest gap / largest entry of the column:", worst)
    assert max(worst.values()) <= 1.45e-9, worst                              # measured 1.45e-10
    monkeypatch.delenv("MCX_DESCRIPTOR_FD")
    default = aad.descriptor_tangents(mixed, model, False)[1]                 # the default mode is the complex step
    assert all(np.array_equal(default[k], dc[k]) for k in dc)


def test_a_real_only_closed_form_falls_back_to_four_points(mixed, monkeypatch):
    _, d4 = aad.descriptor_tangents(mixed, mixed.model, False, mode="4")
    atom = cases.BlackScholesModel._atom

    def real_only(self, req, asset_id):
        math.exp(self._pf(2))                                                 # TypeError at theta + i h
        return atom(self, req, asset_id)
    monkeypatch.setattr(cases.BlackScholesModel, "_atom", real_only)
    with pytest.raises(TypeError):
        aad._descriptors_like(mixed, mixed.model, False, None, np.complex128, complex_step=(0, 1e-30))
    _, dd = aad.descriptor_tangents(mixed, mixed.model, False, mode="complex")
    assert all(np.array_equal(dd[k], d4[k]) for k in d4)


def test_pad_chunk():
    a = np.arange(2 * 3 * 6, dtype=np.float64).reshape(2, 3, 6)
    full, last = aad.pad_chunk(a, [0, 1, 2, 3]), aad.pad_chunk(a, [4, 5])
    assert full.shape == last.shape == (2, 3, NP) and full.flags.c_contiguous and last.flags.c_contiguous
    assert np.array_equal(full, a[..., :4]) and np.array_equal(last[..., :2], a[..., 4:]) and not last[..., 2:].any()


# ---- slots of the analytic Black-Scholes exposure events ---------------------------------------------------------------------------------
def test_bs_exposure_slots(oracle):
    ns, model, rm = cases.bs_european_exposure()                              # European options on an equity, EPE / PFE / PV
    sc = cases.SimulationController(ns, model, rm, 64, 0, 2, cases.E, backend=oracle)
    sc.run_simulation()
    kind = sc.book_plan.events["kind"]
    bs_rows = np.flatnonzero(kind == _abi.EV_EXPO_BS)
    assert len(bs_rows) >= 1 and len(bs_rows) < len(kind)
    assert [p._bs_param_indices(model) for p in sc.products] == [(0, 1, 2)] * 3          # (spot, sigma, rate)
    for sel, want in (([0, 1, 2], (1, 2)), ([0, 2], (-1, 1)), ([1], (0, -1)), ([0], (-1, -1))):
        table = aad._bs_exposure_slots(sc, sc, sel)
        assert table.shape == (len(kind), 2) and table.dtype == np.int32
        assert (table[bs_rows] == want).all(), (sel, table[bs_rows])
        assert (np.delete(table, bs_rows, axis=0) == -1).all()
    assert aad._bs_exposure_slots(cases_mixed_without_bs_events(oracle), None, [0]) is None


def cases_mixed_without_bs_events(oracle):
    ns, model, rm = cases.irs_cva()
    sc = cases.SimulationController(ns, model, rm, 64, 64, 2, cases.E, backend=oracle)
    sc.run_simulation()
    assert not (sc.book_plan.events["kind"] == _abi.EV_EXPO_BS).any()
    return sc


# ---- metric scatter ----------------------------------------------------------------------------------------------------------------------
def test_metric_scatter_writes_the_columns_of_its_chunk_only():
    P, sel, n_dates, N = 6, [4, 5], 3, 48
    rng = np.random.default_rng(5)
    sums = rng.normal(size=(n_dates, 2, NP))                                  # what mcx_tangent_profiles returns: sums over the paths
    asked = []

    def tangent_profiles(rows, threshold, expo, ns_i, delayed, coll):
        asked.append((ns_i, threshold, delayed, coll))
        return sums.copy()
    ns = SimpleNamespace(is_collateralized=lambda: False, threshold=0.25, counterparty_id=None)
    sc = SimpleNamespace(netting_sets=[ns, ns], risk_metrics=SimpleNamespace(metrics=[cases.EPEMetric(), cases.CEMetric()]), num_paths_mainsim=N)
    ctx = aad._BookPass(sc, None, SimpleNamespace(tangent_profiles=tangent_profiles), SimpleNamespace(all_reduce_np=lambda a: a), False, False,
                        False, np.arange(n_dates, dtype=np.int32), None)
    grads = [[[[0.0] * P for _ in range(n_dates)], [[0.0] * P]] for _ in range(2)]
    aad._scatter_metric_tangents(ctx, aad._Chunk(sel, None, None, None, None, None), aad._Images(None, None, None, "expo"), grads)
    assert asked == [(0, 0.25, None, False), (1, 0.25, None, False)]          # one profile tangent per netting set and chunk
    prof = sums / float(N)
    for per_ns in grads:
        epe, ce = np.array(per_ns[0]), np.array(per_ns[1])
        assert np.array_equal(epe[:, 4:], prof[:, 0, :2]) and np.array_equal(ce[:, 4:], prof[:1, 0, :2])
        assert not epe[:, :4].any() and not ce[:, :4].any()
    ene = [[[[0.0] * P for _ in range(n_dates)], [[0.0] * P]]]
    sc.netting_sets, sc.risk_metrics.metrics = [ns], [cases.ENEMetric(), cases.EEPEMetric()]
    aad._scatter_metric_tangents(ctx, aad._Chunk([1], None, None, None, None, None), aad._Images(None, None, None, "expo"), ene)
    assert [row[1] for row in ene[0][0]] == list(prof[:, 1, 0]) and ene[0][1][0][1] == float(prof[:, 0, 0].mean())
    assert sum(v != 0.0 for m in ene[0] for row in m for v in row) == n_dates + 1


# ---- gates -------------------------------------------------------------------------------------------------------------------------------
class _UserCVA(cases.CVAMetric):
    _native = False


def _large(oracle, metric, scheme=cases.E):
    cfg = large_cva_cases.SMALL
    ns, model, _ = large_cva_cases.build(cfg["num_europeans"], cfg["num_bonds"], cfg["num_swaps"], cfg["exposure_timeline"])
    rm = cases.RiskMetrics([metric(large_cva_cases.COUNTERPARTY_ID, 0.4)], exposure_timeline=cfg["exposure_timeline"])
    return cases.SimulationController(ns, model, rm, 64, 64, 2, scheme, differentiate=True, backend=oracle)


def test_gates_report_the_earliest_reason(oracle):
    """72 products on a backend without mcx_tangent_lsm_batch ("products") under a metric the library does not reduce ("metric") and,
    in the third controller, a scheme without dual paths ("scheme"): the reason is that of the first gate in the order second order,
    scheme, metric, products, exercise products, analytic shortcuts"""
    assert not hasattr(oracle, "tangent_lsm_batch")
    for sc, reason in ((_large(oracle, _UserCVA), "metric"), (_large(oracle, cases.CVAMetric), "products"),
                       (_large(oracle, _UserCVA, cases.A), "scheme")):
        assert len(sc.products) == 72
        with pytest.raises(aad._NoTangentForm) as e:
            aad._tangent_book_routes(sc)
        assert str(e.value) == reason
        sc.requires_higher_order_derivatives = True
        with pytest.raises(aad._NoTangentForm, match="second order"):
            aad._tangent_book_routes(sc)


def test_routes_of_a_book_the_pass_takes():
    hip_like = SimpleNamespace(tangent_paths_chol=None, tangent_paths_s2f=None, tangent_lsm_step=None, tangent_lsm_batch=None)
    for build, scheme, want in ((cases.mixed_cva, cases.E, (False, False, False)), (cases.american, cases.A, (False, True, False))):
        ns, model, rm = build()
        sc = cases.SimulationController(ns, model, rm, 64, 64, 1, scheme, differentiate=True, backend=hip_like)
        assert aad._tangent_book_routes(sc) == want
        sc.batch_tangent_lsm = True
        assert aad._tangent_book_routes(sc) == want[:2] + (True,)


def test_no_tangent_form_is_the_library_status():
    from mcx._native import McxError
    assert aad.no_tangent_form(McxError("mcx_tangent_eval: event 3 has no tangent form", _abi.E_NOT_FUSABLE))
    assert not aad.no_tangent_form(McxError("mcx_tangent_eval failed (-2)", -2)) and not aad.no_tangent_form(RuntimeError("(-10)"))
