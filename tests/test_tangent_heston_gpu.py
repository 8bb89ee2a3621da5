"""Forward-mode sensitivities of Heston books on the GPU (csrc/kt_book.hip kt_paths_heston behind mcx_tangent_paths_heston, driven by
mcx.aad.run_with_tangent_book under SimulationController.tangent_heston).

  1. the kernel on injected draws against the long-double restatement of the dual step maps (tests/heston_tangent_reference.py):
     EULER, QE hard and QE smoothed, both parameter sets, all 7 parameters in two chunks (the second zero-padded), 1 / 255 / 257 paths
     in tensors with a padded leading dimension, 6 sub-steps with two distinct dt and 3 stored dates, one of them the calibration
     date.  The inputs meet the margin condition of the fixtures (asserted here, on the CPU); no path is left out.
     Bound: the restatement's own rounding — the largest gap between its float64 and its longdouble run over exactly these inputs,
     relative to a row's largest entry (GAP below) — times 4.  The value image against HipBackend.generate_paths on the same draws;
  2. the kernel on its own Philox draws: any split of the path range gives the same bytes, under EULER and under QE (the uniform's
     counter block included);
  3. every return code of the entry point, with nothing written;
  4. a European PV book through run_with_tangent_book against run_with_tangents (kt_heston): two independent kernels;
  5. end to end against the reference's autograd (fixtures of tests/heston_aad_cases.py), the unchanged bump route with the flag off,
     forward against bumped gradients, three emulated ranks."""
import numpy as np
import pytest
import torch

import cases
import heston_aad_cases as hcases
import heston_tangent_reference as hr
from mcx import _abi, aad
from mcx._native import McxError
from mcx.plan import SimPlan
from test_oracle_golden import check_lsm_sensitivities

pytestmark = pytest.mark.gpu
NP = _abi.TANGENT_NP
TIMELINE = np.array([0.0, 0.25, 1.0])        # three sub-steps per interval: dt = 1/12 and 1/4; date 0 is the calibration date
SIZES = [1, 255, 257]
# float64 against longdouble run of the restatement, largest gap relative to a row's largest entry over the 18 inputs below:
# measured 6.7e-13 (high-psi parameters, QE hard, 255 paths: the tangent of a variance next to the mass at zero); 2.0e-13 for the
# Feller set under QE at one path, below 2e-14 for every EULER input.  Worst device gap measured on the MI355X: 4.4e-13 (the same
# high-psi input; 1.8e-14 smoothed high-psi, 1.3e-14 Feller QE, 9e-16 EULER); the value image equalled generate_paths bit for bit.
GAP = 6.7e-13
BOUND = 4.0 * GAP

# (parameter set, scheme, smoothing) -> (scale of the normals, range of the uniforms).  EULER: the normals are scaled so that no
# path reaches the variance floor; smoothed QE with the high-psi set: uniforms next to one, where u > p on every path-step — below p
# the smoothed mass-at-zero weight times a negative tail takes the variance below zero and the path is NaN
INPUTS = {
    ("feller", "EULER", False): (0.25, None), ("feller", "QE", False): (1.0, (0.02, 0.98)), ("feller", "QE", True): (1.0, (0.02, 0.98)),
    ("highpsi", "EULER", False): (0.03, None), ("highpsi", "QE", False): (1.0, (0.02, 0.98)), ("highpsi", "QE", True): (1.0, (0.98, 0.9995)),
}
PARAMS = {"feller": hcases.FELLER, "highpsi": hcases.HIGHPSI}


def _ld(n):
    return (n + 63) // 64 * 64 + 64


def _padded(hip, a, ld, fill=7.0):
    """the array a [..][n] on the device as a view of a buffer with leading dimension ld, the padding poisoned"""
    buf = torch.full(a.shape[:-1] + (ld,), fill, dtype=torch.float64, device=hip.device)
    buf[..., :a.shape[-1]] = hip.from_numpy(a)
    return buf, buf[..., :a.shape[-1]]


def _setup(hip, pname, scheme, smoothing):
    model = cases.HestonModel(0.0, *PARAMS[pname])
    model.perform_smoothing = smoothing
    plan = SimPlan(model, TIMELINE, getattr(cases.SimulationScheme, scheme), 3)
    assert plan.n_steps == 6 and plan.n_dates == 3 and plan.n_initial_store == 1 and len({round(float(d), 12) for d in plan.steps["dt"]}) == 2
    d0, dd = hcases.bare_tables(model, plan, smoothing)
    assert np.array_equal(d0["aux"], plan.aux) and np.allclose(d0["chol"], plan.chol, rtol=1e-15, atol=1e-16)
    return model, plan, hip.sim_create(plan), hr.tables_of(plan, d0, dd, smoothing), dd


def _draws(plan, key, n):
    zscale, urange = INPUTS[key]
    rng = np.random.default_rng(100 + n)
    z = rng.normal(size=(plan.n_steps, 2, n)) * zscale
    u = rng.uniform(*urange, size=(plan.n_steps, n)) if urange else None
    return z, u


@pytest.fixture(scope="module")
def restated():
    """the restatement's float64 and longdouble runs of every input, computed once: {(key, n): (paths, dpaths, paths_ld, dpaths_ld, margins)}"""
    return {}


def _restate(restated, key, n, plan, tb):
    if (key, n) not in restated:
        z, u = _draws(plan, key, n)
        p64, dp64, mar = hr.dual_paths(tb, z, u, np.float64)
        pl, dpl, _ = hr.dual_paths(tb, z, u, np.longdouble)
        restated[(key, n)] = (p64, dp64, pl, dpl, mar)
    return restated[(key, n)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("key", list(INPUTS), ids=lambda k: f"{k[0]}-{k[1]}-{'smoothed' if k[2] else 'hard'}")
def test_kernel_against_the_long_double_restatement(key, n, hip, restated):
    pname, scheme, smoothing = key
    model, plan, sim, tb, dd = _setup(hip, pname, scheme, smoothing)
    z, u = _draws(plan, key, n)
    p64, dp64, pl, dpl, mar = _restate(restated, key, n, plan, tb)
    assert hr.margins_hold(mar), mar                                           # no path on a band edge, at the floor or on a kink
    own = max(hr.rounding_gap(p64, pl), hr.rounding_gap(dp64, dpl))
    print(f"{key} n={n}: restatement float64 vs longdouble = {own:.3e}; margins {mar}")
    assert own <= GAP                                                          # the measured yardstick still holds for these inputs
    if smoothing and pname == "highpsi" and n > 1:                             # path-steps strictly inside each fuzzy band: the
        assert mar["in_band_psi"] >= 10 and mar["in_band_u"] >= 10, mar        # indicators' own tangents are not zero there
    ld = _ld(n)
    z_buf, d_z = _padded(hip, z, ld)
    u_buf, d_u = _padded(hip, u, ld) if u is not None else (None, None)
    primal = hip.generate_paths(sim, 0, 0, n, inject_z=hip.from_numpy(z), inject_u=hip.from_numpy(u) if u is not None else None).cpu().numpy()
    P = len(model.get_model_params())
    assert P == 7
    for sel in ([0, 1, 2, 3], [4, 5, 6]):
        d = {k: aad.pad_chunk(v, sel) for k, v in dd.items()}
        out = (torch.full((plan.n_dates, 2, ld), 7.0, dtype=torch.float64, device=hip.device),
               torch.full((NP, plan.n_dates, 2, ld), 7.0, dtype=torch.float64, device=hip.device))
        hip.tangent_paths_heston(sim, d["slots"], d["init"], d["aux"], d["chol"], 0, 0, n, d_z, d_u,
                                 out=(out[0][..., :n], out[1][..., :n]), ld=ld)
        hip.synchronize()
        assert bool((out[0][..., n:] == 7.0).all()) and bool((out[1][..., n:] == 7.0).all())      # the padding is not written
        paths, dpaths = out[0][..., :n].cpu().numpy(), out[1][..., :n].cpu().numpy()
        same = paths.tobytes() == primal.tobytes()
        value_gap = float(np.max(np.abs(paths - primal) / np.maximum(np.abs(primal), 1e-300)))
        print(f"{key} n={n} chunk {sel}: value image equals generate_paths bit for bit: {same}; largest relative gap {value_gap:.3e}")
        assert np.allclose(paths, primal, rtol=1e-10, atol=0.0)
        assert hr.rounding_gap(paths, pl) <= BOUND
        for q in range(NP):
            if q >= len(sel):                                                  # the padding of the last chunk: zero in, zero out
                assert not dpaths[q].any(), (key, n, q)
                continue
            gap = hr.rounding_gap(dpaths[q], dpl[sel[q]])
            print(f"{key} n={n} d/d theta_{sel[q]}: worst gap / row's largest entry = {gap:.3e}")
            assert gap <= BOUND, (key, n, sel[q], gap)
    assert np.abs(dpl[:, 1:]).max(axis=(1, 2, 3)).min() > 0.0                   # every parameter moves some stored state


# ---- Philox ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["EULER", "QE"])
def test_split_launches_give_the_bytes_of_one_launch(scheme, hip):
    model, plan, sim, tb, dd = _setup(hip, "feller", scheme, True)
    n, seed = 257, 43
    primal = hip.generate_paths(sim, seed, 0, n).cpu().numpy()
    d = {k: aad.pad_chunk(v, [0, 1, 2, 3]) for k, v in dd.items()}
    args = (sim, d["slots"], d["init"], d["aux"], d["chol"], seed)
    paths, dpaths = hip.tangent_paths_heston(*args, 0, n)
    assert np.allclose(paths.cpu().numpy(), primal, rtol=1e-10, atol=0.0)
    assert float(dpaths.abs().max()) > 0.0 and not bool(torch.isnan(dpaths).any())
    p0, dp0 = hip.tangent_paths_heston(*args, 0, 100)
    p1, dp1 = hip.tangent_paths_heston(*args, 100, 157)
    assert torch.cat([p0, p1], dim=2).cpu().numpy().tobytes() == paths.cpu().numpy().tobytes()
    assert torch.cat([dp0, dp1], dim=3).cpu().numpy().tobytes() == dpaths.cpu().numpy().tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _refused(hip, model, scheme, n=64, dchol="zeros", ld=None, inject="none"):
    """call mcx_tangent_paths_heston on zero derivative tables and poisoned outputs; returns the error after checking that nothing
    was written"""
    plan = SimPlan(model, TIMELINE, scheme, 1)
    sim = hip.sim_create(plan)
    out = (torch.full((plan.n_dates, plan.n_state, n), 7.0, dtype=torch.float64, device=hip.device),
           torch.full((NP, plan.n_dates, plan.n_state, n), 7.0, dtype=torch.float64, device=hip.device))
    z = hip.zeros(plan.n_steps, 2, n) if inject != "none" else None
    u = hip.zeros(plan.n_steps, n) if inject == "both" else None
    lib = hip.lib
    a = [np.zeros((1, _abi.SLOT_NPARAM, NP)), np.zeros((2, NP)), np.zeros((plan.n_steps, 1, _abi.AUX, NP)), np.zeros((max(len(plan.chol), 1), 2, 2, NP))]
    rc = lib.mcx_tangent_paths_heston(hip.h, sim.ptr, _abi.ptr(a[0]), _abi.ptr(a[1]), _abi.ptr(a[2]), _abi.ptr(a[3]) if dchol == "zeros" else None,
                                      43, 0, n, out[0].data_ptr(), out[1].data_ptr(), n if ld is None else ld,
                                      z.data_ptr() if z is not None else None, u.data_ptr() if u is not None else None, hip._stream())
    hip.synchronize()
    assert bool((out[0] == 7.0).all()) and bool((out[1] == 7.0).all())
    msg = lib.mcx_last_error(hip.h)
    return rc, (msg.decode() if msg else "")


def test_refusals(hip):
    who = "mcx_tangent_paths_heston:"
    feller = cases.HestonModel(0.0, *hcases.FELLER)
    assert _refused(hip, feller, cases.E, dchol=None)[0] == -1                 # EULER needs the factor's tangent
    for scheme in (cases.E, cases.Q):
        rc, msg = _refused(hip, feller, scheme, ld=63)
        assert rc == -2 and who in msg and "ld < n_paths" in msg, (rc, msg)
    rc, msg = _refused(hip, feller, cases.Q, inject="z")
    assert rc == -3 and who in msg and "inject_u required" in msg, (rc, msg)
    # every NULL argument on its own, under both schemes (h_dchol only under EULER: QE does not read it)
    for scheme in (cases.E, cases.Q):
        plan = SimPlan(feller, TIMELINE, scheme, 1)
        sim = hip.sim_create(plan)
        out = (torch.full((plan.n_dates, 2, 64), 7.0, dtype=torch.float64, device=hip.device),
               torch.full((NP, plan.n_dates, 2, 64), 7.0, dtype=torch.float64, device=hip.device))
        tabs = [np.zeros((1, _abi.SLOT_NPARAM, NP)), np.zeros((2, NP)), np.zeros((plan.n_steps, 1, _abi.AUX, NP)), np.zeros((1, 2, 2, NP))]
        full = [hip.h, sim.ptr] + [_abi.ptr(x) for x in tabs] + [43, 0, 64, out[0].data_ptr(), out[1].data_ptr(), 64, None, None, hip._stream()]
        nullable = {0: "h", 1: "sim", 2: "h_dslot", 3: "h_dinit", 4: "h_daux", 9: "d_paths", 10: "d_dpaths"}
        for pos, what in nullable.items():
            args = list(full)
            args[pos] = None
            assert hip.lib.mcx_tangent_paths_heston(*args) == -1, (scheme, what)
        args = list(full)
        args[5] = None
        assert hip.lib.mcx_tangent_paths_heston(*args) == (-1 if scheme == cases.E else 0), scheme
        hip.synchronize()
        if scheme == cases.E:
            assert bool((out[0] == 7.0).all()) and bool((out[1] == 7.0).all())
    for model, scheme in ((cases.VasicekModel(0.0, 0.02, 0.04, 0.3, 0.015, asset_id="r"), cases.E), (cases.BlackScholesModel(0.0, 100.0, 0.03, 0.25), cases.A)):
        plan = SimPlan(model, TIMELINE, scheme, 1)
        sim = hip.sim_create(plan)
        out = (torch.full((plan.n_dates, plan.n_state, 64), 7.0, dtype=torch.float64, device=hip.device),
               torch.full((NP, plan.n_dates, plan.n_state, 64), 7.0, dtype=torch.float64, device=hip.device))
        a = [np.zeros((1, _abi.SLOT_NPARAM, NP)), np.zeros((2, NP)), np.zeros((plan.n_steps, 1, _abi.AUX, NP)), np.zeros((max(len(plan.chol), 1), 2, 2, NP))]
        rc = hip.lib.mcx_tangent_paths_heston(hip.h, sim.ptr, *[_abi.ptr(x) for x in a], 43, 0, 64, out[0].data_ptr(), out[1].data_ptr(), 64, None,
                                              None, hip._stream())
        hip.synchronize()
        msg = hip.lib.mcx_last_error(hip.h).decode()
        assert rc == _abi.E_NOT_FUSABLE and who in msg and "a single Heston slot expected" in msg, (rc, msg)
        assert bool((out[0] == 7.0).all()) and bool((out[1] == 7.0).all())
    # the binding raises the library's status
    plan = SimPlan(feller, TIMELINE, cases.Q, 1)
    with pytest.raises(McxError) as e:
        hip.tangent_paths_heston(hip.sim_create(plan), np.zeros((1, _abi.SLOT_NPARAM, NP)), np.zeros((2, NP)), np.zeros((plan.n_steps, 1, _abi.AUX, NP)),
                                 None, 43, 0, 64, hip.zeros(plan.n_steps, 2, 64), None)
    assert e.value.code == -3


# ---- a European PV book: the book pass against the fused tangent kernel ---------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["QE", "EULER"])
def test_book_pass_against_the_fused_tangent_kernel(scheme, hip):
    n, steps = 512, 4

    def build():
        model = cases.HestonModel(0.0, *hcases.FELLER)
        call = cases.EuropeanOption(cases.Equity(), 1.0, 95.0, cases.OptionType.CALL)
        call.name = "call"
        put = cases.EuropeanOption(cases.Equity(), 0.5, 105.0, cases.OptionType.PUT)
        put.name = "put"
        ns = [cases.NettingSet(name="call", products=[call]), cases.NettingSet(name="put", products=[put])]
        sc = cases.SimulationController(ns, model, cases.RiskMetrics([cases.PVMetric()]), n, 0, steps, getattr(cases.SimulationScheme, scheme),
                                        differentiate=True, backend=hip)
        sc.tangent_heston = True
        plan = SimPlan(model, sc.simulation_timeline.numpy(), sc.simulation_scheme, steps)
        rng = np.random.default_rng(5)
        z = rng.normal(size=(plan.n_steps, 2, n)) * (0.25 if scheme == "EULER" else 1.0)
        u = rng.uniform(0.02, 0.98, size=(plan.n_steps, n)) if scheme == "QE" else None
        sc._inject["main"] = (hip.from_numpy(z), hip.from_numpy(u) if u is not None else None)
        return sc

    fused, book = build(), build()
    assert aad.tangent_kernels_apply(fused) and aad.heston_route(book)
    r_f = aad.run_with_tangents(fused)
    r_b = aad.run_with_tangent_book(book)
    assert fused.timings["tangent"] is True and book.timings["forward_mode_passes"] == 2
    g = {"param_names": np.array(r_f.model_param_names)}
    for ns_i in range(2):
        pv_f, pv_b = r_f.results[ns_i][0][0][0], r_b.results[ns_i][0][0][0]
        print(f"{scheme} ns {ns_i}: PV fused {pv_f:.15e} book {pv_b:.15e}; gradients fused {r_f.derivatives[ns_i][0][0]} book {r_b.derivatives[ns_i][0][0]}")
        assert abs(pv_f - pv_b) <= 1e-12 * abs(pv_f)
        g[f"result_{ns_i}_0"] = np.array([[pv_f, 0.0]])
        g[f"grad_{ns_i}_0"] = np.array([r_f.derivatives[ns_i][0][0]], dtype=np.float64)
    check_lsm_sensitivities(book, g, r_b)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
FIXTURES = hcases.fixture_names()


def test_the_fixtures_are_there():
    assert {"heston_american_qe_aad", "heston_netting_euler_aad"} <= set(FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_forward_mode_against_reference_autograd(name, hip):
    sc, g = hcases.make_controller(name, hip, tangent_heston=True)
    res = sc.run_simulation()
    assert sc.timings["tangent"] is True and sc.timings["forward_mode_passes"] == 2 and "bumped_passes" not in sc.timings
    for key in [k for k in g.files if k.startswith("grad_")]:
        ns_i, m_i = (int(x) for x in key.split("_")[1:])
        ref, ours = g[key], np.array(res.derivatives[ns_i][m_i], dtype=np.float64)
        scale = np.abs(ref).max(axis=1, keepdims=True)
        print(f"{name} {key}: worst gap / row's largest entry = {np.max(np.abs(ours - ref) / np.where(scale == 0, 1.0, scale)):.3e}")
    check_lsm_sensitivities(sc, g, res)


@pytest.mark.parametrize("name", FIXTURES)
def test_forward_mode_with_the_quadratic_regression_against_the_host_restatement(name, hip):
    """the controller's default degree 2 on the fixture's draws: a quadratic basis term and a coefficient tangent row for S^2 in every
    regression.  The yardstick is the float64 host restatement of the whole pipeline (tests/heston_book_reference.py), which the
    host tests tie to the reference's tape at degree 1 and to its own long-double run at degree 2 (the tape itself is 4e-6 .. 5e-5
    of a row off there: tests/test_tangent_heston_host.py).  Every row under check_lsm_sensitivities"""
    import heston_book_reference as hb
    sc, g = hcases.make_controller(name, hip, tangent_heston=True, degree=2)
    res = sc.run_simulation()
    assert sc.timings["tangent"] is True and sc.timings["forward_mode_passes"] == 2 and sc.regression_function.degree == 2
    want = hb.run_fixture(name, g, degree=2)
    ref = {"param_names": g["param_names"]}
    for ns_i, per_ns in enumerate(want.results):
        for m_i, evals in enumerate(per_ns):
            ref[f"result_{ns_i}_{m_i}"] = np.array(evals, dtype=np.float64)
            ref[f"grad_{ns_i}_{m_i}"] = np.array(want.derivatives[ns_i][m_i], dtype=np.float64)
            ours = np.array(res.derivatives[ns_i][m_i], dtype=np.float64)
            scale = np.abs(ref[f"grad_{ns_i}_{m_i}"]).max(axis=1, keepdims=True)
            gap = np.max(np.abs(ours - ref[f"grad_{ns_i}_{m_i}"]) / np.where(scale == 0, 1.0, scale))
            tape = np.max(np.abs(ours - g[f"deg2_grad_{ns_i}_{m_i}"]) / np.where(scale == 0, 1.0, scale))
            print(f"{name} degree 2, metric {m_i}: forward against the host restatement {gap:.3e}; against the reference's tape {tape:.3e}")
    check_lsm_sensitivities(sc, ref, res)


@pytest.mark.parametrize("name", FIXTURES)
def test_with_the_flag_off_the_book_is_bumped_as_before(name, hip):
    sc, g = hcases.make_controller(name, hip)
    assert sc.tangent_heston is False
    sc.run_simulation()
    assert sc.timings["tangent"] is False and sc.timings["bumped_passes"] == 14


def test_forward_gradients_agree_with_bumped_gradients_for_the_american_put(hip):
    """the bound is the bump's own truncation, as documented for the American put of the ANALYTICAL section: 4e-6 of the row"""
    name = "heston_american_qe_aad"
    fwd, _ = hcases.make_controller(name, hip, tangent_heston=True)
    bump, _ = hcases.make_controller(name, hip)
    g_f, g_b = fwd.run_simulation().derivatives, bump.run_simulation().derivatives
    assert fwd.timings["tangent"] is True and bump.timings["tangent"] is False
    for m_i in range(len(g_f[0])):
        a, b = np.array(g_f[0][m_i], dtype=np.float64), np.array(g_b[0][m_i], dtype=np.float64)
        scale = np.abs(b).max(axis=1, keepdims=True)
        gap = np.abs(a - b) / np.where(scale == 0, 1.0, scale)
        print(f"{name} metric {m_i}: forward against bumped, worst gap / row's largest entry = {gap.max():.3e}")
        assert np.all(gap <= 4e-6), (m_i, gap.max())


def test_netting_case_on_three_emulated_ranks_matches_the_single_shard_run(hip):
    from emulated_ranks import run_ranks
    from mcx import _native

    def build(be):
        sc, _ = hcases.make_controller("heston_netting_euler_aad", be, inject=False, tangent_heston=True)
        sc.materialize = False
        return sc

    def grads(res):
        return [[np.array(m, dtype=np.float64) for m in per_ns] for per_ns in res.derivatives]

    single = build(hip)
    ref = grads(single.run_simulation())
    assert single.timings["tangent"] is True

    def body(sc, rank):
        g = grads(sc.run_simulation())
        assert sc.timings["tangent"] is True
        return g

    out, calls = run_ranks(3, lambda rank: build(_native.HipBackend(0)), body)
    assert calls["all_reduce"] > 0
    for rank, got in enumerate(out):
        for ns_r, ns_g in zip(ref, got):
            for m_r, m_g in zip(ns_r, ns_g):
                assert np.allclose(m_g, m_r, rtol=1e-9, atol=1e-12), (rank, np.abs(m_g - m_r).max())
