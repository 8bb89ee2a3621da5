"""Forward-mode sensitivities of FVAMetric end to end on the GPU, through run_simulation() with SimulationController.tangent_fva = True:
against the reference's autograd gradient (tests/golden/fva_irs_aad.npz), against the bump route of the same controller, against the
EPE tangents of the same forward run, on three emulated ranks and under a single Vasicek model.  1,024 + 1,024 paths.

Bounds: the fixture's values at fva_cases.assert_meets_golden, its gradients at test_oracle_golden.check_lsm_sensitivities; forward
against bumped at 4e-6 of a row's largest entry, the bound of tests/test_xva_tangent_gpu.py (the bump's own truncation); ranks at rtol
1e-9; the EPE identity at 1e-10 of the row's largest entry, the bound its bumped form has in tests/test_fva_gpu.py (both sides are
sums of the same per-path tangents, only the order of the additions separates them).

The bump route as a yardstick (tests/test_xva_tangent_gpu.py, README "The bump route as a yardstick").  A central difference is the
derivative only while no path crosses relu's kink inside the bump, and at 512 + 512 paths the default Philox seeds carry a path of this
book across it.  So the comparisons run on the seeds one further (seed_offset = 1), every one first ASSERTS that the bump route agrees
with itself at half its step to 1e-6 of the row (a condition on the yardstick, from the yardstick alone), and one test per book keeps
the default seeds and holds the forward route to the half-step bumps at the same 4e-6.  Measured on the MI355X at the 1,024 + 1,024
paths of this module: standard against half step 1.5e-10 to 1.2e-8 on either seeds (no path crosses at this size), forward against
bumped 7.2e-11 to 6.2e-9 (seed_offset = 1) and 8.5e-11 to 1.5e-8 (default seeds, half step), forward against the reference's autograd
on the fixture's draws 1.1e-8."""
import numpy as np
import pytest

import cases
import fva_cases as fc
import fva_reference as fr
import xva_cases as xc
from mcx import _abi, _native, aad
from mcx.metrics.bcva_metric import BilateralCVAMetric
from mcx.metrics.cva_metric import CVAMetric
from mcx.metrics.fva_metric import FVAMetric, funding_weights
from mcx.models.vasicek import VasicekModel
from mcx.products.swap import IRSType
from test_oracle_golden import check_lsm_sensitivities

pytestmark = pytest.mark.gpu
NP = _abi.TANGENT_NP
N = 1024
BUMP_BOUND = 4e-6
BUMP_SELF = 1e-6               # the bump route against itself at half its step, before it is used as a yardstick
SEED_OFFSET = 1                # Philox seeds 43 / 44 (see the module docstring)


def fva(cp="cp", own="own", borrow=fr.BORROW_CURVE, lend=fr.LEND_CURVE):
    return FVAMetric(borrow, lend, counterparty_id=cp, own_id=own)


def _controller(hip, metrics, flag, seed_offset=SEED_OFFSET, xva_flag=False, n=N, **kw):
    sc = xc.controller(hip, metrics, n_main=n, n_pre=n, differentiate=True, **kw)
    sc.tangent_fva, sc.tangent_xva, sc.seed_offset = flag, xva_flag, seed_offset
    return sc


def _four_metrics():
    return [fva(), BilateralCVAMetric("cp", "own", xc.R_CP, xc.R_OWN), CVAMetric("cp", xc.R_CP), cases.EPEMetric()]


def _two_sets(hip, flag, seed_offset=SEED_OFFSET):
    """the payer swap against "cp" and a receiver swap against another counterparty; a metric that names "cp" and one that names
    only the own name"""
    other = xc.netting_sets(irs_type=IRSType.RECEIVER, counterparty_id="someone_else")[0]
    other.name = "other"
    rm = xc.RiskMetrics([fva(), fva(cp=None)], exposure_timeline=xc.TIMELINE)
    sc = xc.SimulationController(xc.netting_sets() + [other], xc.models(), rm, N, N, 2, cases.E, differentiate=True, backend=hip)
    sc.materialize, sc.tangent_fva, sc.seed_offset = True, flag, seed_offset
    return sc


KINDS = ("plain", "collateralised", "four metrics", "two netting sets")


def _book(hip, kind, flag, seed_offset=SEED_OFFSET):
    """the four books of the comparison with the bump route.  "four metrics" holds a bilateral CVA: both flags go together"""
    if kind == "two netting sets":
        return _two_sets(hip, flag, seed_offset)
    if kind == "four metrics":
        return _controller(hip, _four_metrics(), flag, seed_offset, xva_flag=flag)
    kw = dict(threshold=xc.THRESHOLD, mpor=xc.MPOR) if kind == "collateralised" else {}
    return _controller(hip, [fva()], flag, seed_offset, **kw)


def _grads(res):
    return [[np.array(m, dtype=np.float64) for m in per_ns] for per_ns in res.derivatives]


def _forward(sc):
    res = sc.run_simulation()
    P = len(sc.model.get_model_params())
    assert sc.timings["tangent"] is True and sc.timings["forward_mode_passes"] == -(-P // NP) and "bumped_passes" not in sc.timings
    return res


def _bumped(sc):
    res = sc.run_simulation()
    assert sc.timings["tangent"] is False and sc.timings["bumped_passes"] == 2 * len(sc.model.get_model_params())
    return res


def _row_gap(a, b):
    worst = 0.0
    for per_a, per_b in zip(_grads(a), _grads(b)):
        for x, y in zip(per_a, per_b):
            scale = np.abs(y).max(axis=1, keepdims=True)
            worst = max(worst, float((np.abs(x - y) / np.where(scale == 0, 1.0, scale)).max()))
    return worst


def _half_step(monkeypatch):
    step = aad.bump_size
    monkeypatch.setattr(aad, "bump_size", lambda theta: 0.5 * step(theta))


def _yardstick(tag, build_off, monkeypatch):
    """the bump route at its standard step, after it has agreed with itself at half the step"""
    bump = _bumped(build_off())
    with monkeypatch.context() as mp:
        _half_step(mp)
        half = _bumped(build_off())
    own = _row_gap(bump, half)
    print(f"FVA-TANGENT {tag}: bump route, standard against half step, worst gap / row's largest entry = {own:.3e}")
    assert own <= BUMP_SELF, (tag, own)
    return bump


def _compare(tag, fwd, bump):
    """forward against bumped, row by row (one evaluation of one metric of one netting set), relative to the row's largest entry"""
    worst = 0.0
    for ns_i, (per_f, per_b) in enumerate(zip(_grads(fwd), _grads(bump))):
        for m_i, (a, b) in enumerate(zip(per_f, per_b)):
            assert a.shape == b.shape
            scale = np.abs(b).max(axis=1, keepdims=True)
            gap = np.abs(a - b) / np.where(scale == 0, 1.0, scale)
            assert not a[np.broadcast_to(scale == 0, a.shape)].any(), (tag, ns_i, m_i)        # a zero row of the bumps is a zero row
            worst = max(worst, float(gap.max()))
            assert np.all(gap <= BUMP_BOUND), (tag, ns_i, m_i, float(gap.max()))
    print(f"FVA-TANGENT {tag}: forward against bumped, worst gap / row's largest entry = {worst:.3e}")
    for a, b in zip(fwd.results, bump.results):                                               # the values are the base run's on both routes
        for va, vb in zip(a, b):
            assert np.allclose(np.array(va, dtype=np.float64), np.array(vb, dtype=np.float64), rtol=1e-12, atol=0.0)


def test_forward_mode_against_the_reference_autograd(hip):
    g = cases.load_golden("fva_irs_aad")
    borrow = dict(zip(g["borrow_tenors"].tolist(), g["borrow_spreads"].tolist()))
    lend = dict(zip(g["lend_tenors"].tolist(), g["lend_spreads"].tolist()))
    sc = xc.controller(hip, [fva(borrow=borrow, lend=lend)], n_main=g["z_main"].shape[1], n_pre=g["z_pre"].shape[1],
                       timeline=g["metric_exposure_timeline"], differentiate=True)
    sc.tangent_fva = True
    for key, z in (("main", g["z_main"]), ("pre", g["z_pre"])):
        sc._inject[key] = (hip.from_numpy(np.ascontiguousarray(np.transpose(z, (0, 2, 1)))), None)
    assert aad.fva_route(sc) and not aad.xva_route(sc)
    res = sc.run_simulation()
    assert sc.timings["tangent"] is True and sc.timings["forward_mode_passes"] == 3 and "bumped_passes" not in sc.timings
    fc.assert_meets_golden(sc, res, g)
    ours, ref = np.array(res.derivatives[0][0], dtype=np.float64), g["grad_0_0"]
    scale = np.abs(ref).max(axis=1, keepdims=True)
    print(f"FVA-TANGENT golden: worst |forward - autograd| / row's largest entry = {float((np.abs(ours - ref) / scale).max()):.3e}")
    check_lsm_sensitivities(sc, g, res)
    assert ours.shape == (3, 12) and (ours != 0.0).all()                        # both names weigh both legs


def test_a_metric_that_names_only_the_counterparty_has_zero_own_columns(hip):
    res = _forward(_controller(hip, [fva(own=None)], True))
    g = _grads(res)[0][0]
    names = list(res.model_param_names)
    own, cp = [k for k, s in enumerate(names) if s.startswith("own.")], [k for k, s in enumerate(names) if s.startswith("cp.")]
    assert len(own) == 4 and len(cp) == 4
    assert (g[:, own] == 0.0).all() and (g[:, cp] != 0.0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_forward_against_the_bump_route(kind, hip, monkeypatch):
    on, off = _book(hip, kind, True), _book(hip, kind, False)
    assert aad.fva_route(on) and not aad.fva_route(off)
    fwd = _forward(on)
    _compare(kind, fwd, _yardstick(kind, lambda: _book(hip, kind, False), monkeypatch))
    g = _grads(fwd)
    if kind == "four metrics":
        assert g[0][0].shape[0] == 3 and g[0][1].shape[0] == 5 and g[0][3].shape[0] == len(xc.TIMELINE)
    if kind == "two netting sets":
        assert not g[1][0].any() and g[1][0].shape == g[0][0].shape              # gated by the counterparty: three exact-zero rows
        assert np.abs(g[1][1]).max() > 0 and np.abs(g[0][0]).max() > 0      # the metric without a counterparty applies to both


@pytest.mark.parametrize("kind", KINDS)
def test_default_seeds_against_the_half_step_bumps(kind, hip, monkeypatch):
    """the default Philox seeds, where the standard step can carry a path across relu's kink (module docstring): every book's forward
    route against the bump route at half its step, at the same bound"""
    fwd = _forward(_book(hip, kind, True, seed_offset=0))
    full = _bumped(_book(hip, kind, False, seed_offset=0))
    with monkeypatch.context() as mp:
        _half_step(mp)
        half = _bumped(_book(hip, kind, False, seed_offset=0))
    print(f"FVA-TANGENT default seeds, {kind}: bump route standard against half step {_row_gap(full, half):.3e}, "
          f"forward against standard step {_row_gap(fwd, full):.3e}")
    _compare(f"default seeds, {kind}, half step", fwd, half)


def test_fva_and_bilateral_cva_need_both_flags(hip):
    """one flag of the two: the book bumps as it did before either existed"""
    for fva_flag, xva_flag in ((True, False), (False, True)):
        _bumped(_controller(hip, _four_metrics(), fva_flag, xva_flag=xva_flag, n=256))


def test_flag_off_takes_the_bump_route(hip):
    sc = _controller(hip, [fva()], False, n=256)
    assert sc.tangent_fva is False and not aad.fva_route(sc)
    res = sc.run_simulation()
    assert sc.timings["tangent"] is False and sc.timings["bumped_passes"] == 2 * len(sc.model.get_model_params())
    assert np.isfinite(_grads(res)[0][0]).all()


def test_flat_spread_without_names_is_the_sum_of_the_epe_tangents(hip):
    """with no names and a flat spread on the equally spaced timeline every borrowing weight is the same c, so
    d fca = c sum_{k<E-1} d EPE_k of the EPEMetric in the same forward run (kt_fva against kt_profiles: the same per-path tangents,
    another kernel and another order of additions)"""
    s = 0.0125
    sc = _controller(hip, [FVAMetric(s), cases.EPEMetric(), cases.ENEMetric()], True)
    res = _forward(sc)
    P = len(sc.model.get_model_params())
    w = funding_weights(s, xc.TIMELINE)
    assert len(set(w)) == 1 and w[0] > 0.0
    g, g_epe, g_ene = (np.array(res.derivatives[0][k], dtype=np.float64) for k in range(3))
    assert g.shape == (3, P) and g_epe.shape == (len(xc.TIMELINE), P)
    for name, row, want in (("fca", g[0], w[0] * g_epe[:-1].sum(axis=0)), ("fba", g[1], -w[0] * g_ene[:-1].sum(axis=0))):
        scale, gap = float(np.abs(row).max()), float(np.abs(row - want).max())
        print(f"FVA-TANGENT flat spread: d {name} against c * sum d E{'P' if name == 'fca' else 'N'}E, largest gap {gap:.3e} = "
              f"{gap / scale:.3e} of the largest entry")
        assert scale > 0.0 and gap <= 1e-10 * scale


def test_unnamed_metric_under_a_single_vasicek_model(hip, monkeypatch):
    model = lambda: VasicekModel(0.0, 0.03, 0.03, 0.1, 0.01, asset_id="irs")
    build = lambda flag: _controller(hip, [fva(None, None), cases.EPEMetric()], flag, model=model())
    fwd = build(True)
    res = fwd.run_simulation()
    assert fwd.timings["tangent"] is True and fwd.timings["forward_mode_passes"] == 1 and len(fwd.model.get_model_params()) == 4
    _compare("vasicek", res, _yardstick("vasicek", lambda: build(False), monkeypatch))
    g, g_epe = _grads(res)[0]
    wb = np.array(funding_weights(fr.BORROW_CURVE, xc.TIMELINE))
    want = wb @ g_epe[:-1]
    assert np.abs(g[0]).max() > 0 and np.abs(g[0] - want).max() <= 1e-10 * np.abs(g[0]).max()


def test_three_emulated_ranks_reproduce_one_shard(hip, monkeypatch):
    import emulated_ranks
    n_main, n_pre = 1501, 1000

    def build(be):
        sc = xc.controller(be, [fva(), fva(None, None)], n_main=n_main, n_pre=n_pre, threshold=xc.THRESHOLD, mpor=xc.MPOR, differentiate=True)
        sc.materialize, sc.tangent_fva = False, True
        return sc

    sums = []
    plain = emulated_ranks.EmulatedShard.all_reduce_np

    def counted(self, a):
        if self.rank == 0 and np.shape(a) == (3, 1 + NP):
            sums.append(1)
        return plain(self, a)
    monkeypatch.setattr(emulated_ranks.EmulatedShard, "all_reduce_np", counted)
    ref = _grads(_forward(build(hip)))
    out, calls = emulated_ranks.run_ranks(3, lambda rank: build(_native.HipBackend(0)), lambda sc, rank: _forward(sc))
    assert len(sums) == 3 * 2                       # one all-reduce of the 15 sums per netting set (1), metric (2) and pass (3)
    for rank, got in enumerate(out):
        for m_i, (a, b) in enumerate(zip(ref[0], _grads(got)[0])):
            assert np.abs(a).max() > 0 and np.allclose(a, b, rtol=1e-9, atol=0.0), (rank, m_i, a, b)
