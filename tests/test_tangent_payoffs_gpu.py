"""Forward-mode sensitivities of the payoff forms on the GPU (csrc/kt_book.hip kt_payoff_event / kt_barrier_event behind
mcx_book_set_payoff_tangents, driven by mcx.aad.run_with_tangent_book with SimulationController.tangent_payoffs).

  1. kernel level: mcx_tangent_eval, mcx_tangent_lsm and mcx_tangent_lsm_batch on an armed book against the numpy restatement
     (tests/payoff_tangent_reference.py) per path and per parameter slot, at 1, 255 and 257 paths with a padded leading dimension;
     the value image against mcx_eval_book on the same paths and uniforms.
     Bound: the restatement's own rounding — the largest gap between its float64 and its longdouble run, relative to the row's
     largest entry, measured over exactly these inputs: 4.2e-14 (the 2-asset geometric basket at one path; 1.7e-14 for the bridge,
     3e-16 for binary and plain barriers) — times 4, for the few ulps each mcx_log / mcx_exp adds and the bridge chains;
  2. the bridge on its own Philox uniforms, recomputed on the host from the counters, at two path offsets; split launches give the
     bytes of one launch;
  3. a disarmed book refuses with MCX_E_NOT_FUSABLE and writes nothing, armed it is taken, disarmed again it refuses again; an armed
     book without such events returns the bytes of the disarmed call (the old instantiation);
  4. end to end against the reference's autograd (fixtures of tests/payoff_aad_cases.py), the opt-in flag against the bump route,
     three emulated ranks on the bridge book with Philox draws."""
import copy

import numpy as np
import pytest

import payoff_aad_cases as pcases
from mcx import _abi
from mcx._native import McxError
from mcx.aad import stateless_lsm_jobs
from payoff_tangent_reference import PayoffRestatement, philox_bridge_uniforms, rounding_gap
from test_oracle_golden import check_lsm_sensitivities

pytestmark = pytest.mark.gpu
NP = _abi.TANGENT_NP
GAP = 4.2e-14                                 # measured: see the module docstring
BOUND = 4.0 * GAP
EPS = np.finfo(np.float64).eps
SIZES = [1, 255, 257]


def _ld(n):
    return (n + 63) // 64 * 64 + 64


def _pad(a, ld, fill=1.0):
    out = np.full(a.shape[:-1] + (ld,), fill)
    out[..., :a.shape[-1]] = a
    return out


class _Device:
    """a fresh book of `sc`'s plan on the device with the host-made inputs of n paths in tensors of leading dimension ld"""

    def __init__(self, hip, sc, n, seed, philox=None):
        self.hip, self.plan, self.n, self.ld = hip, sc.book_plan, n, _ld(n)
        sim = sc.sim_plan
        self.x = x = pcases.kernel_inputs(self.plan, sim.n_state, sim.n_dates, n, seed)
        if philox is not None:                # (seed, path offset): the bridge draws its own uniforms
            ev = self.plan.events
            for q in range(len(ev)):
                if ev["kind"][q] == _abi.EV_OPTION and ev["aux"][q][0] == 5.0:
                    draw = int(self.plan.coeffs[ev["coeff_off"][q] + 1])
                    x["bridge"][draw] = philox_bridge_uniforms(philox[0], philox[1], n, int(ev["term_end"][q] - ev["term_begin"][q]) - 1, draw)
        self.book = hip.book_create(self.plan)
        self.paths, self.dpaths = hip.from_numpy(_pad(x["paths"], self.ld)), hip.from_numpy(_pad(x["dpaths"], self.ld, 0.0))
        self.datoms, self.dpayoff = hip.from_numpy(x["datoms"]), hip.from_numpy(x["dpayoff"])
        self.coeffs, self.dcoeffs = hip.zeros(max(len(self.plan.coeffs), 1)), hip.zeros(max(len(self.plan.coeffs), 1), NP)
        self.inject = {k: hip.from_numpy(_pad(u, self.ld, 0.5)) for k, u in x["bridge"].items()}
        if philox is not None:
            hip.book_set_bridge_rng(self.book, philox[0], philox[1], None)
        elif self.inject:
            hip.book_set_bridge_rng(self.book, 0, 0, self.inject)

    def restatement(self, dtype=np.float64):
        x = self.x
        return PayoffRestatement(self.plan, x["paths"], x["dpaths"], x["datoms"], x["dpayoff"], x["bridge"], dtype=dtype)

    def arm(self, on=True):
        self.hip.book_set_payoff_tangents(self.book, self.dpayoff if on else None)

    def eval(self, out=None):
        cfs, _expo = self.hip.tangent_eval(self.book, self.datoms, self.coeffs, self.dcoeffs, self.paths, self.dpaths, n_paths=self.n, out=out)
        return cfs.cpu().numpy()[..., :self.n]

    def jobs(self, sc):
        lsm_plan, _ = sc._regression_plan()
        x_ids = sorted({x for _, _, _, atoms in lsm_plan for _, x in atoms})
        stats = self.hip.lsm_stats(self.book, x_ids, self.paths[:, :, :self.n])
        table, _ = stateless_lsm_jobs(lsm_plan, {x: (stats[i, 0], stats[i, 1]) for i, x in enumerate(x_ids)}, sc._expo_coeff_base, self.plan.n_basis)
        return table

    def lsm(self, q):
        return self.hip.tangent_lsm(self.book, int(q["product"]), int(q["first_event"]), int(q["num_atom"]), int(q["x_atom"]), float(q["shift"]),
                                    float(q["scale"]), self.datoms, self.paths, self.dpaths, n_paths=self.n)

    def lsm_batch(self, table, out=None):
        return self.hip.tangent_lsm_batch(self.book, table, self.datoms, self.paths, self.dpaths, n_paths=self.n, out=out)


@pytest.fixture(scope="module")
def pv_books(hip):
    return {name: pcases.kernel_controller(name, hip) for name in pcases.KERNEL_BOOKS}


@pytest.fixture(scope="module")
def expo_books(hip):
    return {name: pcases.kernel_controller(name, hip, exposures=True) for name in pcases.KERNEL_BOOKS + ["plain"]}


def _rows_within(got, want, bound, what):
    scale = np.max(np.abs(want), axis=-1, keepdims=True)
    gap = np.abs(got - want)
    worst = float(np.max(gap / np.where(scale == 0, 1.0, scale)))
    print(f"{what}: worst device gap / row's largest entry = {worst:.3e} (bound {bound:.3e})")
    assert np.all(gap <= bound * scale), (what, worst)
    return worst


# ---- 1. kernel level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", pcases.KERNEL_BOOKS)
def test_eval_against_the_restatement(name, n, pv_books, hip):
    d = _Device(hip, pv_books[name], n, 7)
    rs = d.restatement()
    want = rs.cashflows()
    assert rs.smallest_margin() > 1e-9                                         # no path on a band edge, a kink or a tie
    gap = rounding_gap(lambda dt: d.restatement(dt).cashflows())
    print(f"{name} n={n}: restatement float64 vs longdouble = {gap:.3e}")
    assert gap <= GAP                                                          # the measured yardstick still holds for these inputs
    if name == "cv":
        assert d.x["dpayoff"].any()                                            # the control variate's own tangent row is not zero
    d.arm()
    got = d.eval()
    d.arm(False)
    assert got.shape == want.shape == (1 + NP, len(d.plan.products), n)
    assert n == 1 or np.abs(want[1:]).max() > 0.0                              # (one path may well pay nothing)
    _rows_within(got, want, BOUND, f"{name} n={n}")
    primal, _ = hip.eval_book(d.book, d.paths[:, :, :n])                       # same paths, same injected uniforms
    assert np.allclose(got[0], primal.cpu().numpy()[:, :n], rtol=1e-10, atol=1e-12), (name, n)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", pcases.KERNEL_BOOKS)
def test_lsm_and_batch_against_the_restatement(name, n, expo_books, hip):
    sc = expo_books[name]
    d = _Device(hip, sc, n, 11)
    table = d.jobs(sc)
    assert len(table) >= 2
    rs, K = d.restatement(), d.plan.n_basis
    d.arm()
    single = np.stack([d.lsm(q) for q in table])
    batch = d.lsm_batch(table)
    d.arm(False)
    assert batch.tobytes() == single.tobytes()                                 # the batch is the single call, bit for bit
    worst = 0.0
    for j, q in enumerate(table):
        t = rs.moments(int(q["product"]), int(q["first_event"]), int(q["num_atom"]), int(q["x_atom"]), float(q["shift"]), float(q["scale"]), K, terms=True)
        want = t.sum(axis=-1)
        # every summand within BOUND of its row's largest, n of them; any summation order within n eps of the sum of magnitudes
        tol = n * BOUND * np.abs(t).max(axis=-1) + n * EPS * np.abs(t).sum(axis=-1)
        gap = np.abs(single[j] - want)
        worst = max(worst, float(np.max(gap / np.where(tol == 0, 1.0, tol))))
        assert np.all(gap <= tol), (name, n, j, float(np.max(gap / np.where(tol == 0, 1.0, tol))))
    assert rs.smallest_margin() > 1e-9
    print(f"{name} n={n}: {len(table)} jobs, worst moment gap / tolerance = {worst:.3e}")


# ---- 2. the bridge on Philox uniforms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, (1 << 32) + 5])
def test_bridge_on_philox_uniforms(offset, pv_books, hip):
    n, seed = 257, 43
    d = _Device(hip, pv_books["bridge"], n, 13, philox=(seed, offset))
    rs = d.restatement()
    want = rs.cashflows()
    assert rs.smallest_margin() > 1e-9
    # the hit pattern these uniforms make: on a good share of the paths some interval's fuzzy hit clamp((p - u + 0.05) / 0.1, 0, 1) is
    # non-zero, and the uniforms of another counter range give another payoff image and other tangents
    hit_paths = sum(int(h.sum()) for h in rs.hits.values())
    assert len(rs.hits) == len(d.x["bridge"]) and hit_paths >= n // 10, (len(rs.hits), hit_paths)
    other = dict(d.x, bridge={k: philox_bridge_uniforms(seed, offset + 1000, n, u.shape[0] // 2, k) for k, u in d.x["bridge"].items()})
    moved = PayoffRestatement(d.plan, other["paths"], other["dpaths"], other["datoms"], other["dpayoff"], other["bridge"]).cashflows()
    assert np.abs(moved[0] - want[0]).max() > 1e-3 and np.abs(moved[1:] - want[1:]).max() > 1e-3
    d.arm()
    got = d.eval()
    _rows_within(got, want, BOUND, f"bridge philox offset {offset}")
    primal, _ = hip.eval_book(d.book, d.paths[:, :, :n])
    assert np.allclose(got[0], primal.cpu().numpy()[:, :n], rtol=1e-10, atol=1e-12)
    # two launches over [0, 130) and [130, 257) with their own path offsets: the bytes of the one launch
    parts = []
    for lo, hi in ((0, 130), (130, n)):
        hip.book_set_bridge_rng(d.book, seed, offset + lo, None)
        cfs, _ = hip.tangent_eval(d.book, d.datoms, d.coeffs, d.dcoeffs, d.paths[:, :, lo:hi].contiguous(), d.dpaths[:, :, :, lo:hi].contiguous())
        parts.append(cfs.cpu().numpy())
    d.arm(False)
    assert np.concatenate(parts, axis=-1).tobytes() == np.ascontiguousarray(got).tobytes()


# ---- 3. armed and disarmed -----------------------------------------------------------------------------------------------------------
def test_a_disarmed_book_refuses_and_writes_nothing(expo_books, hip):
    sc = expo_books["binary"]
    n = 255
    d = _Device(hip, sc, n, 17)
    table = d.jobs(sc)
    n_ns, rows = d.plan.n_netting_sets, max(d.plan.n_expo_rows, 1)

    def refused():
        cfs, expo = hip.zeros(1 + NP, n_ns, d.ld) + 7.0, hip.zeros(1 + NP, n_ns, rows, d.ld) + 7.0
        mom = np.full((len(table), 1 + NP, 3 * d.plan.n_basis - 1), 7.0)
        for call in (lambda: d.eval(out=(cfs, expo)), lambda: d.lsm(table[0]), lambda: d.lsm_batch(table, out=mom)):
            with pytest.raises(McxError) as e:
                call()
            assert e.value.code == _abi.E_NOT_FUSABLE and "has no tangent form" in str(e.value), str(e.value)
        hip.synchronize()
        assert bool((cfs == 7.0).all()) and bool((expo == 7.0).all()) and (mom == 7.0).all()

    refused()                                                                  # the state after mcx_book_create
    d.arm()
    got = d.eval()
    assert np.isfinite(got).all() and np.abs(got[1:]).max() > 0.0
    assert np.isfinite(d.lsm(table[0])).all() and np.isfinite(d.lsm_batch(table)).all()
    d.arm(False)
    refused()                                                                  # NULL again: the same refusal


def test_an_armed_book_without_payoff_events_runs_the_old_instantiation(expo_books, hip):
    sc = expo_books["plain"]
    ev = sc.book_plan.events
    assert not ((ev["kind"] == _abi.EV_OPTION) & (ev["aux"][:, 0] != 0.0)).any()
    d = _Device(hip, sc, 257, 19)
    table = d.jobs(sc)
    d.coeffs, d.dcoeffs = hip.from_numpy(np.random.default_rng(3).normal(0.0, 0.5, len(d.plan.coeffs))), hip.from_numpy(
        np.random.default_rng(4).normal(0.0, 0.1, (len(d.plan.coeffs), NP)))
    out = {}
    for armed in (False, True):
        d.arm(armed)
        cfs, expo = hip.tangent_eval(d.book, d.datoms, d.coeffs, d.dcoeffs, d.paths, d.dpaths, n_paths=d.n)
        out[armed] = (cfs.cpu().numpy()[..., :d.n].tobytes(), expo.cpu().numpy()[..., :d.n].tobytes(), d.lsm_batch(table).tobytes())
    d.arm(False)
    assert out[True] == out[False]


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------
def _grads(res):
    return [[np.array(m, dtype=np.float64) for m in per_ns] for per_ns in res.derivatives]


@pytest.mark.parametrize("name", list(pcases.CASES))
def test_forward_mode_against_reference_autograd_and_the_bump_route(name, hip):
    sc, g = pcases.make_controller(name, hip, tangent_payoffs=True)
    res = sc.run_simulation()
    P = len(sc.model.get_model_params())
    assert sc.timings["tangent"] is True and sc.timings["forward_mode_passes"] == -(-P // NP) and "bumped_passes" not in sc.timings
    check_lsm_sensitivities(sc, g, res)
    off, _ = pcases.make_controller(name, hip, tangent_payoffs=False)          # the default: the library refuses, the run is bumped
    res_off = off.run_simulation()
    assert off.timings["tangent"] is False and off.timings["bumped_passes"] == 2 * P
    # forward against bump-and-revalue, under the bump's own truncation as the existing forward-vs-bump tests hold it: rtol 5e-5 and
    # 3e-5 of the row's largest entry for a bumped path that crosses a band edge or a kink
    worst = 0.0
    for ns_f, ns_b in zip(_grads(res), _grads(res_off)):
        for m_f, m_b in zip(ns_f, ns_b):
            scale = np.abs(m_f).max()
            worst = max(worst, float(np.max(np.abs(m_f - m_b)) / scale))
            assert scale > 0 and np.allclose(m_b, m_f, rtol=5e-5, atol=3e-5 * scale), (name, m_f, m_b)
    print(f"{name}: forward vs bump, worst gap / row's largest entry = {worst:.3e}")


def test_bridge_book_through_a_pre_simulation_against_the_bump_route(hip):
    """a bridge barrier with EPE through a pre-simulation, Philox draws: the dual regression must draw the pre-simulation's bridge
    uniforms (seed, path range) and the dual main pass the main simulation's, chunk after chunk — with the book's bridge state left
    at the other simulation's, the regressed coefficients or the payoff image are those of other uniforms.  The bump route sets the
    state in the primal controller; forward and bumped gradients under the bound of the fixtures above"""
    import cases
    p = cases.BarrierOption(0.0, 1.0, 100.0, 6, cases.OptionType.CALL, 125.0, cases.BarrierOptionType.UPANDOUT)
    p.name = "bridge"
    p.set_use_brownian_bridge()
    out = {}
    for flag in (True, False):
        model = cases.BlackScholesModel(0, 100.0, 0.03, 0.25)
        q = copy.deepcopy(p)
        rm = cases.RiskMetrics([cases.PVMetric(), cases.EPEMetric()], exposure_timeline=np.array([0.0, 0.4, 0.8]))
        sc = cases.SimulationController([cases.NettingSet(name="b", products=[q])], model, rm, 2048, 2048, 1, cases.A, differentiate=True, backend=hip)
        sc.tangent_payoffs = flag
        res = sc.run_simulation()
        assert sc.timings["tangent"] is flag
        out[flag] = (np.array([v[0] for m in res.results[0] for v in m]), _grads(res)[0])
    assert np.allclose(out[True][0], out[False][0], rtol=1e-12, atol=0.0)         # the same base run under both routes
    worst = 0.0
    for m_f, m_b in zip(out[True][1], out[False][1]):
        scale = np.abs(m_f).max()
        worst = max(worst, float(np.max(np.abs(m_f - m_b)) / scale))
        assert scale > 0 and np.allclose(m_b, m_f, rtol=5e-5, atol=3e-5 * scale), (m_f, m_b)
    print(f"bridge + pre-simulation: forward vs bump, worst gap / row's largest entry = {worst:.3e}")


def test_bridge_book_on_three_emulated_ranks_matches_the_single_shard_run(hip):
    from emulated_ranks import run_ranks
    from mcx import _native

    def build(be):
        sc, _ = pcases.make_controller("payoff_barrier_bridge_aad", be, inject=False, tangent_payoffs=True)
        sc.materialize = False
        return sc

    single = build(hip)
    ref = _grads(single.run_simulation())
    assert single.timings["tangent"] is True

    def body(sc, rank):
        g = _grads(sc.run_simulation())
        assert sc.timings["tangent"] is True
        return g

    out, _calls = run_ranks(3, lambda rank: build(_native.HipBackend(0)), body)
    for rank, got in enumerate(out):
        for ns_r, ns_g in zip(ref, got):
            for m_r, m_g in zip(ns_r, ns_g):
                assert np.allclose(m_g, m_r, rtol=1e-9, atol=1e-12), (rank, np.abs(m_g - m_r).max())
