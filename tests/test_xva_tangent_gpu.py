"""Forward-mode sensitivities of DVAMetric / BilateralCVAMetric end to end on the GPU, through run_simulation() with
SimulationController.tangent_xva = True: against the reference's autograd gradient (tests/golden/xva_irs_aad.npz), against the bump
route of the same controller, on three emulated ranks, against the mirrored CVA book, and on the wide dual path route.

Bounds: the fixture's values at xva_cases.assert_meets_golden, its gradients at test_oracle_golden.check_lsm_sensitivities; forward
against bumped at 4e-6 of a row's largest entry, the bump's own truncation (tests/test_wide_tangent_gpu.py, tests/test_hw_tangent_gpu.py
hold their routes to the same); ranks and mirror at rtol 1e-9.

The bump route as a yardstick.  A central difference is the derivative only while no path crosses a kink inside the bump.  With the
default Philox seeds at 512 + 512 paths, path 349 of this book has the exposure -3.34e-7 on metric date 3, and the bump of irs.rate
(h = 1e-5 x 0.03 = 3e-7, d exposure / d rate ~ 2) carries it across relu's kink: one summand of 512 changes legs.  There the bump route
at its standard step and at half of it differ by 7.6e-5 (plain) and 1.7e-4 (collateralised) of the row's largest entry in that column
(CPU oracle and MI355X alike: the same Philox paths), and the forward route differs from the standard step by exactly those figures —
7.595e-5 / 1.671e-4 / 4.03e-4 (five metrics: an EPE row) / 7.595e-5 (two netting sets) measured on the MI355X — while it agrees with the half step, and with the reference's
autograd on the fixture's draws at 8.0e-9.  So the comparisons below run on the Philox seeds one further (seed_offset = 1: smallest
|exposure| 2.6e-6, standard against half step 1.2e-8 / 2.3e-8), every one first ASSERTS that the bump route agrees with itself at
half its step to 1e-6 of the row (a quarter of the bound; a condition on the yardstick, from the yardstick alone), and one test per
book keeps the default seeds and holds the forward route to the half-step bumps at the same 4e-6."""
import numpy as np
import pytest

import cases
import xva_cases as xc
from mcx import _abi, _native, aad
from mcx.metrics.bcva_metric import BilateralCVAMetric
from mcx.metrics.cva_metric import CVAMetric
from mcx.metrics.dva_metric import DVAMetric
from mcx.products.swap import IRSType
from test_oracle_golden import check_lsm_sensitivities

pytestmark = pytest.mark.gpu
NP = _abi.TANGENT_NP
BUMP_BOUND = 4e-6
BUMP_SELF = 1e-6               # the bump route against itself at half its step, before it is used as a yardstick
SEED_OFFSET = 1                # Philox seeds 43 / 44 (see the module docstring)


def bcva():
    return BilateralCVAMetric("cp", "own", xc.R_CP, xc.R_OWN)


def _controller(hip, metrics, flag, n=512, seed_offset=SEED_OFFSET, **kw):
    sc = xc.controller(hip, metrics, n_main=n, n_pre=n, differentiate=True, **kw)
    sc.tangent_xva, sc.seed_offset = flag, seed_offset
    return sc


def _five_metrics():
    return [CVAMetric("cp", xc.R_CP), bcva(), DVAMetric("own", xc.R_OWN), cases.PVMetric(), cases.EPEMetric()]


def _two_sets(hip, flag, seed_offset=SEED_OFFSET):
    """the payer swap against "cp" and a receiver swap against another counterparty, bilateral CVA and DVA"""
    other = xc.netting_sets(irs_type=IRSType.RECEIVER, counterparty_id="someone_else")[0]
    other.name = "other"
    rm = xc.RiskMetrics([bcva(), DVAMetric("own", xc.R_OWN)], exposure_timeline=xc.TIMELINE)
    sc = xc.SimulationController(xc.netting_sets() + [other], xc.models(), rm, 512, 512, 2, cases.E, differentiate=True, backend=hip)
    sc.materialize, sc.tangent_xva, sc.seed_offset = True, flag, seed_offset
    return sc


KINDS = ("plain", "collateralised", "five metrics", "two netting sets")


def _book(hip, kind, flag, seed_offset=SEED_OFFSET):
    """the four books of the comparison with the bump route, at 512 + 512 Philox paths"""
    if kind == "two netting sets":
        return _two_sets(hip, flag, seed_offset)
    kw = dict(threshold=xc.THRESHOLD, mpor=xc.MPOR) if kind == "collateralised" else {}
    return _controller(hip, _five_metrics() if kind == "five metrics" else [bcva()], flag, seed_offset=seed_offset, **kw)


def _grads(res):
    return [[np.array(m, dtype=np.float64) for m in per_ns] for per_ns in res.derivatives]


def _forward(sc):
    res = sc.run_simulation()
    P = len(sc.model.get_model_params())
    assert sc.timings["tangent"] is True and sc.timings["forward_mode_passes"] == -(-P // NP) and sc.timings.get("bumped_passes", 0) == 0
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
    print(f"XVA-TANGENT {tag}: bump route, standard against half step, worst gap / row's largest entry = {own:.3e}")
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
    print(f"XVA-TANGENT {tag}: forward against bumped, worst gap / row's largest entry = {worst:.3e}")
    for a, b in zip(fwd.results, bump.results):                                               # the values are the base run's on both routes
        for va, vb in zip(a, b):
            assert np.allclose(np.array(va, dtype=np.float64), np.array(vb, dtype=np.float64), rtol=1e-12, atol=0.0)


def test_forward_mode_against_the_reference_autograd(hip):
    g = cases.load_golden("xva_irs_aad")
    sc = xc.controller(hip, [bcva()], n_main=g["z_main"].shape[1], n_pre=g["z_pre"].shape[1], timeline=g["metric_exposure_timeline"],
                       differentiate=True)
    sc.tangent_xva = True
    for key, z in (("main", g["z_main"]), ("pre", g["z_pre"])):
        sc._inject[key] = (hip.from_numpy(np.ascontiguousarray(np.transpose(z, (0, 2, 1)))), None)
    assert aad.xva_route(sc)
    res = sc.run_simulation()
    assert sc.timings["tangent"] is True and sc.timings["forward_mode_passes"] == 3 and sc.timings.get("bumped_passes", 0) == 0
    xc.assert_meets_golden(sc, res, g)
    ours, ref = np.array(res.derivatives[0][0], dtype=np.float64), g["grad_0_0"]
    scale = np.abs(ref).max(axis=1, keepdims=True)
    print(f"XVA-TANGENT golden: worst |forward - autograd| / row's largest entry = {float((np.abs(ours - ref) / scale).max()):.3e}")
    check_lsm_sensitivities(sc, g, res)
    names = list(res.model_param_names)
    own, cp = [k for k, s in enumerate(names) if s.startswith("own.")], [k for k, s in enumerate(names) if s.startswith("cp.")]
    assert len(own) == 4 and len(cp) == 4
    assert (ours[0, own] == 0.0).all() and (ours[1, cp] == 0.0).all() and (ours[2:] != 0.0).all()


@pytest.mark.parametrize("kind", ["plain", "collateralised"])
def test_forward_against_the_bump_route(kind, hip, monkeypatch):
    on, off = _book(hip, kind, True), _book(hip, kind, False)
    assert aad.xva_route(on) and not aad.xva_route(off)
    _compare(kind, _forward(on), _yardstick(kind, lambda: _book(hip, kind, False), monkeypatch))


@pytest.mark.parametrize("kind", KINDS)
def test_default_seeds_against_the_half_step_bumps(kind, hip, monkeypatch):
    """the default Philox seeds, where the standard step carries one path across relu's kink (module docstring): every book's
    forward route against the bump route at half its step, at the same bound"""
    fwd = _forward(_book(hip, kind, True, seed_offset=0))
    full = _bumped(_book(hip, kind, False, seed_offset=0))
    with monkeypatch.context() as mp:
        _half_step(mp)
        half = _bumped(_book(hip, kind, False, seed_offset=0))
    print(f"XVA-TANGENT default seeds, {kind}: bump route standard against half step {_row_gap(full, half):.3e}, "
          f"forward against standard step {_row_gap(fwd, full):.3e}")
    _compare(f"default seeds, {kind}, half step", fwd, half)


def test_whole_book_stays_in_forward_mode(hip, monkeypatch):
    """CVA, bilateral CVA, DVA, PV and EPE in one RiskMetrics: one forward-mode pass serves them all"""
    kind = "five metrics"
    fwd, bump = _forward(_book(hip, kind, True)), _yardstick(kind, lambda: _book(hip, kind, False), monkeypatch)
    _compare(kind, fwd, bump)
    g = _grads(fwd)[0]
    assert g[1].shape[0] == 5 and g[2].shape[0] == 1 and g[4].shape[0] == len(xc.TIMELINE)
    assert g[2][0].tobytes() == g[1][1].tobytes()                               # DVAMetric is the dva record: the same launch arithmetic
    assert np.allclose(g[0][0], g[1][0], rtol=1e-9, atol=0.0)                   # CVAMetric through kt_cva, the cva record through kt_xva


def test_second_netting_set_of_another_counterparty_keeps_zero_rows(hip, monkeypatch):
    kind = "two netting sets"
    fwd, bump = _forward(_book(hip, kind, True)), _yardstick(kind, lambda: _book(hip, kind, False), monkeypatch)
    _compare(kind, fwd, bump)
    g = _grads(fwd)
    assert not g[1][0].any() and g[1][0].shape == g[0][0].shape                  # gated by the counterparty: five exact-zero rows
    assert np.abs(g[1][1]).max() > 0 and np.abs(g[0][0][2:]).min() > 0           # DVA applies to every netting set; the first-to-default rows are full


def test_three_emulated_ranks_reproduce_one_shard(hip, monkeypatch):
    import emulated_ranks
    n_main, n_pre = 1501, 1000

    def build(be):
        sc = xc.controller(be, [bcva(), DVAMetric("own", xc.R_OWN)], n_main=n_main, n_pre=n_pre, threshold=xc.THRESHOLD, mpor=xc.MPOR,
                           differentiate=True)
        sc.materialize, sc.tangent_xva = False, True
        return sc

    sums = []
    plain = emulated_ranks.EmulatedShard.all_reduce_np

    def counted(self, a):
        if self.rank == 0 and np.shape(a) == (5, 1 + NP):
            sums.append(1)
        return plain(self, a)
    monkeypatch.setattr(emulated_ranks.EmulatedShard, "all_reduce_np", counted)
    ref = _grads(_forward(build(hip)))
    out, calls = emulated_ranks.run_ranks(3, lambda rank: build(_native.HipBackend(0)), lambda sc, rank: _forward(sc))
    assert len(sums) == 3 * 2                       # one all-reduce of the 25 sums per netting set (1), metric (2) and chunk (3)
    for rank, got in enumerate(out):
        for m_i, (a, b) in enumerate(zip(ref[0], _grads(got)[0])):
            assert np.allclose(a, b, rtol=1e-9, atol=0.0), (rank, m_i, a, b)


def test_dva_gradient_equals_the_forward_mode_cva_gradient_of_the_mirrored_book(hip):
    sc = _controller(hip, [DVAMetric("own", xc.R_OWN)], True, counterparty_id=None)
    g = _grads(_forward(sc))[0][0][0]
    sc_m = _controller(hip, [CVAMetric("own", xc.R_OWN)], False, counterparty_id=None, irs_type=IRSType.RECEIVER)
    res_m = sc_m.run_simulation()
    assert sc_m.timings["tangent"] is True                                      # CVAMetric has had its dual (kt_cva) all along
    g_m = _grads(res_m)[0][0][0]
    print("dva gradient", g, "mirrored cva gradient", g_m, "largest difference", np.abs(g - g_m).max())
    assert np.abs(g).max() > 0.0 and np.allclose(g, g_m, rtol=1e-9, atol=0.0)
    names = list(res_m.model_param_names)
    assert not g[[k for k, s in enumerate(names) if s.startswith("cp.")]].any()


def test_composes_with_the_wide_route(hip, monkeypatch):
    """the ten-factor CVA book of tests/wide_aad_cases.py with two of its CIR++ names as counterparty and own name: the dual paths
    come from mcx_tangent_paths_wide, the xVA tangents from mcx_tangent_xva"""
    import wide_aad_cases as wa
    import wide_cases as wc
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    mod = wc.mcx_classes()
    a, b = wc.CVA_COUNTERPARTIES[0], wc.CVA_COUNTERPARTIES[1]

    def build(flag):
        ns, model, _rm = wa.cva10_theta(mod)
        rm = mod["RiskMetrics"]([BilateralCVAMetric(f"cp{a}", f"cp{b}", 0.4, 0.35), mod["CVAMetric"](f"cp{a}", 0.4)],
                                exposure_timeline=np.array([0.0, 0.5, 1.0]))
        sc = SimulationController(ns, model, rm, 512, 512, 2, SimulationScheme.EULER, differentiate=True, backend=hip)
        sc.tangent_wide, sc.tangent_xva = True, flag
        return sc
    on, off = build(True), build(False)
    assert aad.wide_route(on) and aad.xva_route(on) and aad.wide_route(off) and not aad.xva_route(off)
    del off
    fwd = on.run_simulation()
    P = len(on.model.get_model_params())
    assert on.timings["tangent"] is True and on.timings["forward_mode_passes"] == -(-P // NP) and on.sim_plan.wide
    bump = _bumped(build(False))             # (default seeds, as the issue states the case: the comparison holds at the standard step)
    _compare("wide", fwd, bump)
    with monkeypatch.context() as mp:
        _half_step(mp)
        print(f"XVA-TANGENT wide: bump route, standard against half step = {_row_gap(bump, _bumped(build(False))):.3e}")
    g = _grads(fwd)
    assert np.abs(g[0][0]).max() > 0 and not g[1][0].any() and not g[2][0].any()          # the other counterparties' sets: zero rows
