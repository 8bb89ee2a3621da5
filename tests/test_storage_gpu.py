"""The gas storage on the GPU (csrc/k6_storage.hip behind mcx_storage_*): inject-Z parity with the reference's fixtures, the
backward-step kernel against plain references, Philox-mode runs of random storages against the numpy restatement
(tests/storage_reference.py) on the GPU's own paths, the reference's anchor values, the one-call pre-simulation, and a run at
262,144 + 262,144 paths.

Decisions are hard (argmax over three actions).  In the fixtures no decision of the reference is closer than min_rel_gap >= 4e-8
while kernel and reference differ by <= 1e-10 relative, so NO path may differ there.  In Philox mode a path may be left out of the
cashflow / exposure comparison only if the restatement itself reports a decision margin below 1e-9 on it, and at most 1e-3 of the
paths of a case."""
import math

import numpy as np
import pytest
import torch

import lsm_reference as R
import storage_cases
from mcx import _abi
from storage_reference import AtomReader, StorageRestatement
from test_storage_reference import storages_of

pytestmark = pytest.mark.gpu
C_MOM = 4.0            # as tests/test_lsm_basis_sizes.py: |m - m_ref| <= C_MOM (2K + log2 n) eps sum|term|
MARGIN, MAX_LEFT_OUT = 1e-9, 1e-3


# ---- inject-Z against the reference's fixtures (tolerances of test_hip_parity._check_against_golden) --------------------------
@pytest.mark.parametrize("name", list(storage_cases.CASES))
def test_inject_z_against_reference(name, hip):
    sc, g = storage_cases.make_controller(name, hip)
    res = sc.run_simulation()
    ours = sc.last_state["paths"].permute(2, 0, 1).cpu().numpy()
    assert np.allclose(ours, g["paths_main"], rtol=1e-11, atol=1e-13), np.abs(ours - g["paths_main"]).max()
    pre = sc.last_state["paths_pre"].permute(2, 0, 1).cpu().numpy()
    assert np.allclose(pre, g["paths_pre"], rtol=1e-11, atol=1e-13)
    for i, p in enumerate(sc.products):
        for key, our_c in ((f"expo_coeffs_{i}", sc.regression_coeffs[i].numpy()), (f"prod_coeffs_{i}", p.regression_coeffs.numpy())):
            if key in g.files and g[key].size:
                ref_c = g[key]
                scale = np.maximum(np.abs(ref_c).max(), 1e-300)
                print(name, key, "max coefficient error / scale", np.abs(our_c - ref_c).max() / scale)
                assert np.allclose(our_c, ref_c, rtol=1e-6, atol=1e-8 * scale), (name, key, np.abs(our_c - ref_c).max())
    for ns_i in range(len(sc.netting_sets)):
        mine = [i for i in range(len(sc.products)) if sc.product_to_netting_set_idx[i] == ns_i]
        cf, ref = sc.last_state["cfs"][ns_i].cpu().numpy(), sum(g[f"cfs_{i}"] for i in mine)
        print(name, ns_i, "cashflows: max error", np.abs(cf - ref).max(), "paths off", int((~np.isclose(cf, ref, rtol=1e-10, atol=1e-12)).sum()))
        assert np.allclose(cf, ref, rtol=1e-10, atol=1e-12)                # every path: no decision differs
        ex, ref = sc.last_state["expo"][ns_i].cpu().numpy(), sum(g[f"exposures_{i}"] for i in mine)
        print(name, ns_i, "exposures: max error", np.abs(ex - ref).max())
        assert np.allclose(ex, ref, rtol=1e-8, atol=1e-10)
        for m_i, metric in enumerate(sc.risk_metrics.metrics):
            ref = g[f"result_{ns_i}_{m_i}"]
            got = np.array([[v, e] for v, e in res.results[ns_i][m_i]], dtype=np.float64)
            assert np.allclose(got[:, 0], ref[:, 0], rtol=1e-8, atol=1e-10), (name, metric.get_name(), got[:, 0], ref[:, 0])
            assert np.allclose(got[:, 1], ref[:, 1], rtol=1e-6, atol=1e-12), (name, metric.get_name(), got[:, 1], ref[:, 1])


# ---- random storages ---------------------------------------------------------------------------------------------------------
def random_storage_controller(seed, hip, S=None, degree=None, n_pre=4096, n_main=4096):
    """a random but satisfiable storage on the gas model: 1-3 windows, 1-4 knots per curve, random costs, S, degree, scheme"""
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    from mcx.maths.regression import PolyomialRegression
    mod = storage_cases.mcx_classes()
    r = np.random.default_rng(seed)
    S = int(r.integers(2, 13)) if S is None else S
    degree = int(r.integers(1, 5)) if degree is None else degree
    end = float(r.choice([6.0, 7.5, 8.0]))
    rollout = float(r.choice([1.0, 1.0, 2.0]))
    for attempt in range(50):
        c = mod["StorageConfig"]()
        n_win = int(r.integers(1, 4))
        cuts = [0.0] + sorted(r.choice(np.arange(1.0, end), size=n_win - 1, replace=False).tolist()) + [end + 1.0]
        for k in range(n_win):
            lo = float(r.uniform(0.0, 3.0)) if k else 0.0
            c.add_volume_constraint(cuts[k], cuts[k + 1], lo, lo + float(r.uniform(4.0, 12.0)), 0.0)
        for add, base in ((c.add_injection_flexibility, -1.0), (c.add_withdrawal_flexibility, 1.0)):
            knots = np.sort(r.uniform(0.0, 12.0, int(r.integers(1, 5))))
            for q, x in enumerate(knots):
                add(0.0, end + 1.0, float(x), float(max(0.3, 2.0 + base * 0.4 * q + r.uniform(-0.3, 0.3))))
        c.add_variable_injection_cost(0.0, float(r.uniform(0.0, 0.4)))
        c.add_variable_injection_cost(float(r.integers(1, 6)), float(r.uniform(0.0, 0.4)))
        c.add_variable_withdrawal_cost(0.0, float(r.uniform(0.0, 0.3)))
        try:
            p = mod["Storage"]("gas", 0.0, end, float(r.uniform(1.0, 4.0)), c, S, rollout)
            break
        except ValueError:
            continue
    else:
        raise AssertionError("no satisfiable storage drawn")
    tl = np.unique(np.concatenate([[0.0, end], r.choice(np.arange(0.5, end, 0.5), size=3, replace=False)]))
    rm = mod["RiskMetrics"]([mod["PVMetric"](), mod["EPEMetric"]()], exposure_timeline=tl)
    scheme = SimulationScheme.ANALYTICAL if seed % 2 == 0 else SimulationScheme.EULER
    sc = SimulationController([mod["NettingSet"](name="st", products=[p])], storage_cases._gas_model(mod), rm, n_main, n_pre, 2, scheme,
                              False, regression_function=PolyomialRegression(degree=degree), backend=hip)
    sc.materialize = True
    return sc


def restate_run(sc, p_i=0):
    """the restatement on the run's own paths (copied to the host)"""
    p, K = sc.products[p_i], sc.regression_function.get_degree()
    asset = p.asset_ids[0]
    pre = AtomReader(sc, sc.last_state["paths_pre"].cpu().numpy())
    main = AtomReader(sc, sc.last_state["paths"].cpu().numpy())
    expo_times = [float(t) for t in sc.exposure_timeline]
    out = []
    for centred in (False, True):          # the reference's regression as it stands, and the same regression solved in a centred basis
        rs = StorageRestatement(p, K, sc.reference_float32_cf_cache, centred=centred)
        back = rs.backward(expo_times, lambda t: pre.spot(asset, t), pre.numeraire)
        prod_coeffs = np.stack([back[t]["coeffs"] for t in rs.dates])
        expo_coeffs = np.stack([back[t]["coeffs"] if t in back else np.zeros((rs.S, K)) for t in expo_times])
        cfs, expo, margin = rs.forward(expo_times, True, lambda t: main.spot(asset, t), main.numeraire, prod_coeffs, expo_coeffs)
        out.append(dict(prod_coeffs=prod_coeffs, expo_coeffs=expo_coeffs, cfs=cfs, expo=expo, margin=margin))
    r = out[0]
    # what the restatement itself does not know about an exposure: least squares on raw monomials of x ~ 30 loses cond(A) eps
    # (~1e-6 at degree 4) in the coefficients; the two solves differ by that much, and so may the kernel from either
    r["expo_own_error"] = np.abs(out[0]["expo"] - out[1]["expo"])
    r["margin"] = np.minimum(out[0]["margin"], out[1]["margin"])
    return r


@pytest.mark.parametrize("seed", range(12))
def test_philox_random_storages_against_the_restatement(seed, hip):
    sc = random_storage_controller(100 + seed, hip)
    sc.run_simulation()
    r = restate_run(sc)
    p = sc.products[0]
    for ours, ref, tag in ((p.regression_coeffs.numpy(), r["prod_coeffs"], "prod"), (sc.regression_coeffs[0].numpy(), r["expo_coeffs"], "expo")):
        scale = np.maximum(np.abs(ref).max(), 1e-300)
        print(seed, tag, "S", p.num_states, "K", ours.shape[2], "max coefficient error / scale", np.abs(ours - ref).max() / scale)
        assert np.allclose(ours, ref, rtol=1e-6, atol=1e-8 * scale), (seed, tag, np.abs(ours - ref).max(), scale)
    keep = r["margin"] >= MARGIN
    left_out = 1.0 - keep.mean()
    cf, ex = sc.last_state["cfs"][0].cpu().numpy(), sc.last_state["expo"][0].cpu().numpy()
    print(seed, "left out", left_out, "min margin", r["margin"].min(), "cashflow error", np.abs(cf - r["cfs"])[keep].max(),
          "paths off", int((~np.isclose(cf, r["cfs"], rtol=1e-10, atol=1e-12)).sum()))
    assert left_out <= MAX_LEFT_OUT
    assert np.allclose(cf[keep], r["cfs"][keep], rtol=1e-10, atol=1e-12)
    err, tol = np.abs(ex - r["expo"])[:, keep], (1e-10 + 1e-8 * np.abs(r["expo"]) + 4.0 * r["expo_own_error"])[:, keep]
    print(seed, "exposure error", err.max(), "restatement's own", r["expo_own_error"][:, keep].max(), "largest exposure", np.abs(r["expo"]).max())
    assert (err <= tol).all(), (seed, (err / tol).max())


# ---- kernel level: one backward step -------------------------------------------------------------------------------------------
# every (S, K) at a path count that is no multiple of 64; three of them also below one block's worth per CU and on the grid-stride loop
STEP_CASES = [(S, K, 4099) for S in (2, 5, 10, 32) for K in (2, 4, 6)] + [(S, K, n) for S, K in ((2, 2), (10, 4), (32, 6)) for n in (1000, 300007)]


@pytest.mark.parametrize("S,K,n_pre", STEP_CASES)
def test_backward_step_moments_and_cache(S, K, n_pre, hip):
    """mcx_storage_lsm_step on random cache contents: the rolled cache against the restatement's step (every path outside the
    decision margin), the moments against lsm_reference.moments_ref on the kernel's own rolled cache — for a middle date, the
    last date (continuation 0), an empty roll and the degenerate first regression date; with and without the float32 buffer"""
    sc = random_storage_controller(7 * S + K, hip, S=S, degree=K - 1, n_pre=n_pre, n_main=256)
    assert sc.regression_function.get_degree() == K
    sc.run_simulation()
    p, st, meta = sc.products[0], sc._storage_handle(0), sc._storage_meta[0]
    paths = sc.last_state["paths_pre"]
    n = paths.shape[2]
    assert n == n_pre
    rs = StorageRestatement(p, K, True)
    rd = AtomReader(sc, paths.cpu().numpy())
    rng = np.random.default_rng(S * 100 + K)
    W_old = hip.from_numpy(rng.normal(50.0, 30.0, (S, n)))
    n_dates = len(rs.dates)
    x_all = hip.resolve_atoms(sc.book, [a_[1] for a_ in meta["action"]], paths).cpu().numpy()
    for roll, reg, flags in ((n_dates // 2, n_dates // 2 - 1, _abi.LSM_F32_CACHE), (n_dates // 2, n_dates // 2 - 1, 0),
                             (n_dates - 1, n_dates - 2, _abi.LSM_F32_CACHE), (-1, n_dates // 2, 0), (1, 0, _abi.LSM_F32_CACHE)):
        num_id, x_id = meta["action"][reg]
        x = x_all[reg]
        degenerate = not (x.max() > x.min())
        assert degenerate == (reg == 0)
        shift, scale = (x.min(), 1.0) if degenerate else (0.5 * (x.min() + x.max()), 2.0 / (x.max() - x.min()))
        W_new = hip.zeros(S, n)
        mom = hip.storage_lsm_step(sc.book, st, roll, num_id, x_id, shift, scale, paths, W_old, W_new, flags=flags).cpu().numpy()
        W_after = (W_new if roll >= 0 else W_old).cpu().numpy()
        if roll >= 0:
            t = rs.dates[roll]
            states = np.tile(np.arange(S, dtype=np.float64), (n, 1))
            ns, cf, margin = rs.step(roll, states, rd.spot("gas", t), rd.numeraire(t), p.regression_coeffs[roll].numpy())
            if flags & _abi.LSM_F32_CACHE:
                cf = cf.astype(np.float32).astype(np.float64)
            from storage_reference import _lerp
            want = (cf + _lerp(W_old.cpu().numpy().T.copy(), ns)).T
            keep = margin.min(axis=1) >= MARGIN
            assert 1.0 - keep.mean() <= MAX_LEFT_OUT, (S, K, roll, keep.mean())
            err = np.abs(W_after - want)[:, keep].max()
            print(S, K, n, "roll", roll, "flags", flags, "cache error", err)
            assert np.allclose(W_after[:, keep], want[:, keep], rtol=1e-11, atol=1e-11), (S, K, roll, err)
        a = hip.resolve_atoms(sc.book, [num_id, x_id], paths).cpu().numpy()
        z = (a[1] - shift) * scale
        ref, mag = R.moments_ref(z, a[0][None, :] * W_after, K)
        bound = C_MOM * (2 * K + math.log2(max(n, 2))) * R.EPS * mag
        assert mom.shape == ref.shape and (np.abs(mom - ref) <= bound).all(), (S, K, n, roll, np.abs(mom - ref) / np.maximum(bound, 1e-300))


# ---- anchors -------------------------------------------------------------------------------------------------------------------
def anchor_controller(name, hip, n_main, n_pre, degree=None):
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    from mcx.maths.regression import PolyomialRegression
    mod = storage_cases.mcx_classes()
    g = storage_cases.load_golden("storage_anchors")
    p, model = storage_cases.anchor_scenario(g, name, mod)
    kw = {} if degree is None else {"regression_function": PolyomialRegression(degree=degree)}
    sc = SimulationController([mod["NettingSet"](name=p.get_name(), products=[p])], model, mod["RiskMetrics"](metrics=[mod["PVMetric"]()]),
                              n_main, n_pre, 1, SimulationScheme.ANALYTICAL, False, backend=hip, **kw)
    return sc, g


def test_zero_volatility_store_is_worth_its_inventory(hip):
    sc, _ = anchor_controller("zero_vol", hip, 2000, 2000)
    pv = sc.run_simulation().results[0][0][0][0]
    assert abs(pv - 10.0) < 1e-3, pv


@pytest.mark.parametrize("name", ["storage1", "storage2"])
def test_reference_scenarios_within_four_sigma(name, hip):
    """another random stream than the reference's: 4 sigma of the two standard errors (the suite's convention for stream-to-stream
    comparisons)"""
    sc, g = anchor_controller(name, hip, 2000, 4000, degree=3)
    pv, se = sc.run_simulation().results[0][0][0]
    ref, se_ref = float(g[name + "_pv"]), float(g[name + "_mc_error"])
    print(name, "pv", pv, "+-", se, "reference", ref, "+-", se_ref, "seconds", sc.timings.get("total"))
    assert abs(pv - ref) <= 4.0 * math.sqrt(se * se + se_ref * se_ref), (name, pv, se, ref, se_ref)


class CountingBackend:
    """passes everything through to the backend and counts the storage entry points"""

    def __init__(self, be):
        self._be, self.calls = be, {}

    def __getattr__(self, name):
        v = getattr(self._be, name)
        if name.startswith("storage_") and callable(v):
            def counted(*a, **k):
                self.calls[name] = self.calls.get(name, 0) + 1
                return v(*a, **k)
            return counted
        return v


def test_single_rank_presimulation_is_one_library_call(hip):
    be = CountingBackend(hip)
    sc, _ = anchor_controller("storage2", be, 2000, 4000, degree=3)
    sc.run_simulation()
    assert be.calls.get("storage_lsm_run") == 1 and "storage_lsm_step" not in be.calls, be.calls
    assert be.calls.get("storage_eval") == 1 and be.calls.get("storage_create") == 1, be.calls


def test_storage2_at_262144_paths(hip):
    """storage2 with PV and a monthly EPE profile: runs to completion, finite results (no timing assertion)"""
    mod = storage_cases.mcx_classes()
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    from mcx.maths.regression import PolyomialRegression
    g = storage_cases.load_golden("storage_anchors")
    p, model = storage_cases.anchor_scenario(g, "storage2", mod)
    rm = mod["RiskMetrics"]([mod["PVMetric"](), mod["EPEMetric"]()], exposure_timeline=np.arange(0.0, 451.0, 30.0))
    sc = SimulationController([mod["NettingSet"](name="st", products=[p])], model, rm, 262144, 262144, 1, SimulationScheme.ANALYTICAL, False,
                              regression_function=PolyomialRegression(degree=3), backend=hip)
    res = sc.run_simulation()
    pv, se = res.results[0][0][0]
    epe = np.array(res.results[0][1], dtype=np.float64)
    print("storage2 at 262144 + 262144 paths: pv", pv, "+-", se, "seconds", sc.timings.get("total"), "epe[:3]", epe[:3, 0])
    assert math.isfinite(pv) and math.isfinite(se) and np.isfinite(epe).all() and len(epe) == 16
    sc.release_device_buffers()
    torch.cuda.empty_cache()
