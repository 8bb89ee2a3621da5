"""Sensitivities through the gas storage on the GPU (csrc/kt_storage.hip behind mcx_tangent_storage_* / mcx_tangent_paths_s2f, driven
by mcx/aad.py run_with_tangent_book).  Every test here fails on a tree without the feature: the constructor refuses
differentiate=True with a Storage, and the three entry points do not exist.

  1. the four fixture cases with injected draws: forward mode, values of the non-differentiated run, gradients against the
     reference's autograd fixture (bounds: test_storage_aad_reference.py) and against the numpy restatement (the value bound of
     test_storage_gpu.py: rtol 1e-8, atol 1e-10 max|row|);
  2. the two storage kernels alone against the restatement at S in {2, 10, 32}, K in {1, 3, 4}, fed with RANDOM path, atom and
     coefficient tangents (the kernels are linear in them): roll / no roll / last date, float32 step buffer on and off; image 0
     against mcx_storage_lsm_step / mcx_storage_eval;
  3. the Schwartz two-factor dual paths, both schemes, against complex-step differentiation of the numpy path restatement;
  4. additivity of PV gradients on storage_mixed; 5. three emulated ranks; 6. refusals; 7. a Schwartz two-factor book WITHOUT a
     storage keeps the differentiation route it had (never the new dual paths)."""
import math

import numpy as np
import pytest
import torch

import storage_cases
import storage_tangent_reference as T
from mcx import _abi
from storage_reference import StorageRestatement, _lerp
from test_storage_aad_reference import check_against_reference, load_aad

pytestmark = pytest.mark.gpu
NP = _abi.TANGENT_NP
MARGIN, MAX_LEFT_OUT = 1e-9, 1e-3            # as test_storage_gpu.py: paths the restatement itself cannot decide are left out
PASSES = {"storage_const": 2, "storage_shift": 2, "storage_short_last": 2, "storage_mixed": 3}


def controller(name, backend, differentiate, inject=True, build=None):
    """storage_cases.make_controller with the differentiate flag (and optionally another book on the case's model and draws)"""
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    from mcx.maths.regression import PolyomialRegression
    b, n_pre, n_main, steps, scheme, degree = storage_cases.CASES[name]
    ns, model, rm = (build or b)(storage_cases.mcx_classes())
    sc = SimulationController(ns, model, rm, n_main, n_pre, steps, getattr(SimulationScheme, scheme), differentiate,
                              regression_function=PolyomialRegression(degree=degree), backend=backend)
    sc.materialize = True
    if inject:
        g = storage_cases.load_golden(name)
        for phase in ("pre", "main"):
            sc._inject[phase] = (backend.from_numpy(np.ascontiguousarray(np.transpose(g["z_" + phase], (0, 2, 1)))), None)
    return sc


def values(res):
    return [[np.array([v[0] for v in m], dtype=np.float64) for m in ns] for ns in res.results]


def gradients(res):
    return [[np.array(m, dtype=np.float64) for m in ns] for ns in res.derivatives]


# ---- 1. the fixture cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(storage_cases.CASES))
def test_fixture_case_gradients(name, hip):
    plain = controller(name, hip, False)
    v0 = values(plain.run_simulation())
    sc = controller(name, hip, True)
    res = sc.run_simulation()
    assert sc.timings["tangent"] is True and sc.timings["forward_mode_passes"] == PASSES[name], sc.timings
    print(name, "differentiated run", sc.timings["total"], "s; plain run", plain.timings.get("total"), "s")
    for a_ns, b_ns in zip(v0, values(res)):
        for a, b in zip(a_ns, b_ns):
            assert np.array_equal(a, b), (name, a, b)
    ga = load_aad(name)
    got = gradients(res)
    for ns_i in range(len(sc.netting_sets)):
        for m_i, m in enumerate(sc.risk_metrics.metrics):
            check_against_reference(name, ga, f"{ns_i}_{m_i}", got[ns_i][m_i], m.get_name() == "pv")
    r = T.restate_case(name, centred=True)
    assert r["grads"]
    for tag, want in r["grads"].items():
        ns_i, m_i = (int(v) for v in tag.split("_"))
        scale = np.abs(want).max(axis=1, keepdims=True)
        err = np.abs(got[ns_i][m_i] - want)
        print(name, tag, "against the restatement: max error / max|row|", (err / np.maximum(scale, 1e-300)).max())
        assert (err <= 1e-8 * np.abs(want) + 1e-10 * scale).all(), (name, tag, (err / np.maximum(scale, 1e-300)).max())


# ---- 2. the kernels alone --------------------------------------------------------------------------------------------------------------
def atom_dual(sc, paths, dpaths, datoms, atom_id):
    """value [n], tangents [NP][n] and the sum of the tangent's |terms| of a book atom from host copies: v = a + d x + b exp(c0 + c1 x)"""
    a = sc.book_plan.atoms[atom_id]
    n = paths.shape[2]
    x = paths[a["t_idx"], a["col"]] if a["col"] >= 0 else np.zeros(n)
    dx = dpaths[:, a["t_idx"], a["col"]] if a["col"] >= 0 else np.zeros((NP, n))
    da = datoms[atom_id][:, :, None]                                        # [5][NP][1]
    E = np.exp(a["c0"] + a["c1"] * x) if a["b"] != 0.0 else np.zeros(n)
    v = a["a"] + a["d"] * x + a["b"] * E
    terms = [da[0] + 0.0 * x, da[1] * x, a["d"] * dx, da[2] * E, a["b"] * E * da[3], a["b"] * E * da[4] * x, a["b"] * E * a["c1"] * dx]
    return v, sum(terms), sum(np.abs(t) for t in terms)


def step_setup(sc, hip, rng, h_datoms, datoms, coeffs, S, K, n_pre):
    """what one dual backward step of the storage of `sc` is checked on: the pre-simulation paths with random tangents, a random old
    cache with random tangents, and both restatements"""
    from types import SimpleNamespace
    p, meta = sc.products[0], sc._storage_meta[0]
    c = SimpleNamespace(sc=sc, hip=hip, S=S, K=K, n=n_pre, st=sc._storage_handle(0), meta=meta, datoms=datoms, coeffs=coeffs, h_datoms=h_datoms,
                        prod_coeffs=p.regression_coeffs.numpy(), rs_p=StorageRestatement(p, K, True), rs=T.StorageTangentRestatement(p, K, True))
    c.paths = sc.last_state["paths_pre"].contiguous()
    c.h_paths = c.paths.cpu().numpy()
    c.h_dpaths = rng.normal(0.0, 0.2, (NP,) + c.h_paths.shape)
    c.dpaths = hip.from_numpy(c.h_dpaths)
    c.W_old, c.dW_old = rng.normal(50.0, 30.0, (S, n_pre)), rng.normal(0.0, 20.0, (NP, S, n_pre))
    c.d_W_old, c.d_dW_old = hip.from_numpy(c.W_old), hip.from_numpy(c.dW_old)
    c.x_all = hip.resolve_atoms(sc.book, [a_[1] for a_ in meta["action"]], c.paths).cpu().numpy()
    return c


def check_step(c, roll, reg, flags):
    """one call of mcx_tangent_storage_lsm_step (roll: the action date rolled or -1, reg: the date regressed on): image 0 against the
    primal step, the cache tangent against the restatement, the dual moments against sums over the kernel's own cache"""
    sc, hip, S, K, n_pre, meta, rs, rs_p = c.sc, c.hip, c.S, c.K, c.n, c.meta, c.rs, c.rs_p
    atom_all = lambda q: atom_dual(sc, c.h_paths, c.h_dpaths, c.h_datoms, q)
    atom = lambda q: atom_all(q)[:2]
    num_id, x_id = meta["action"][reg]
    x = c.x_all[reg]
    shift, scale = (0.5 * (x.min() + x.max()), 2.0 / (x.max() - x.min())) if x.max() > x.min() else (x.min(), 1.0)
    d_W_new, d_dW_new = hip.zeros(S, n_pre), hip.zeros(NP, S, n_pre)
    mom = hip.tangent_storage_lsm_step(sc.book, c.st, roll, num_id, x_id, shift, scale, c.datoms, c.coeffs, c.paths, c.dpaths, c.d_W_old, c.d_dW_old,
                                       d_W_new, d_dW_new, flags=flags)
    W_ref = hip.zeros(S, n_pre)
    mom_ref = hip.storage_lsm_step(sc.book, c.st, roll, num_id, x_id, shift, scale, c.paths, c.d_W_old, W_ref, flags=flags).cpu().numpy()
    W_after = (d_W_new if roll >= 0 else c.d_W_old).cpu().numpy()
    dW_after = (d_dW_new if roll >= 0 else c.d_dW_old).cpu().numpy()
    keep = np.ones(n_pre, dtype=bool)
    if roll >= 0:
        assert np.array_equal(W_after, W_ref.cpu().numpy()), (S, K, roll, "image 0 is the primal step's cache")
        t = rs.dates[roll]
        (spot, dspot), (num, dnum) = atom(meta["action"][roll][1]), atom(meta["action"][roll][0])
        states = np.tile(np.arange(S, dtype=np.float64), (n_pre, 1))
        ns, _cf, margin = rs_p.step(roll, states, spot, num, c.prod_coeffs[roll])
        keep = margin.min(axis=1) >= MARGIN
        assert 1.0 - keep.mean() <= MAX_LEFT_OUT
        ns2, _cf2, dcf = rs.step(roll, states, spot, dspot, num, dnum, c.prod_coeffs[roll])
        want = dcf + T._lerp_fixed(np.transpose(c.dW_old, (0, 2, 1)), ns2, S)                 # [NP][n][S]
        want = np.transpose(want, (0, 2, 1))
        big = np.abs(want).max()
        err = np.abs(dW_after - want)[:, :, keep].max()
        print(S, K, "roll", roll, "flags", flags, "cache tangent error / largest", err / big)
        assert err <= 1e-11 * big, (S, K, roll, flags, err, big)
    assert np.allclose(mom[0], mom_ref, rtol=1e-12, atol=1e-12 * np.abs(mom_ref).max()), (S, K, roll, "image 0 of the moments")
    # dual moments from the kernel's own cache: sums of d(z^k) and of d(z^k num W_s); the bound is the one of the primal moments
    # (test_lsm_basis_sizes.py) on the sum of the |terms| a tangent is made of, eight more roundings for the atoms' chain rule
    (xv, dxv, axv), (num, dnum, anum) = atom_all(x_id), atom_all(num_id)
    z, dz, az = (xv - shift) * scale, dxv * scale, axv * abs(scale)
    NB = 2 * K - 1
    ref, mag = np.zeros((NP, NB + S * K)), np.zeros((NP, NB + S * K))
    for k in range(NB):
        dzk = k * z ** (k - 1) * dz if k else np.zeros_like(dz)
        azk = k * np.abs(z) ** (k - 1) * az if k else np.zeros_like(dz)
        ref[:, k], mag[:, k] = dzk.sum(axis=1), azk.sum(axis=1)
        if k < K:
            for s in range(S):
                term = dzk * (num * W_after[s]) + z ** k * (dnum * W_after[s] + num * dW_after[:, s])
                aterm = azk * np.abs(num * W_after[s]) + np.abs(z) ** k * (anum * np.abs(W_after[s]) + np.abs(num * dW_after[:, s]))
                ref[:, NB + s * K + k], mag[:, NB + s * K + k] = term.sum(axis=1), aterm.sum(axis=1)
    bound = 4.0 * (2 * K + 8 + math.log2(n_pre)) * np.finfo(np.float64).eps * mag + 1e-300
    assert (np.abs(mom[1:] - ref) <= bound).all(), (S, K, roll, (np.abs(mom[1:] - ref) / bound).max())


def test_step_kernel_on_a_full_grid(hip):
    """262,181 paths at S = 10, K = 4: more 256-path tiles (1,025) than the step kernel's grid may hold (four blocks per compute
    unit), so the grid is at its cap, a block strides over more than one tile, and the workspace holds the partial moments of the
    largest grid — the 4,099 paths of the test below make 17 blocks of one tile each.  One roll with the float32 step buffer."""
    from test_storage_gpu import random_storage_controller
    S, K, n_pre = 10, 4, 262_181
    sc = random_storage_controller(11 * S + K, hip, S=S, degree=K - 1, n_pre=n_pre, n_main=256)
    sc.materialize = True
    sc.run_simulation()
    rng = np.random.default_rng(77)
    h_datoms = rng.normal(0.0, 0.3, (len(sc.book_plan.atoms), 5, NP))
    h_datoms[:, 3:] *= 0.1
    c = step_setup(sc, hip, rng, h_datoms, hip.from_numpy(h_datoms), hip.from_numpy(hip.book_get_coeffs(sc.book)), S, K, n_pre)
    n_dates = len(c.rs.dates)
    check_step(c, n_dates // 2, n_dates // 2 - 1, _abi.LSM_F32_CACHE)


@pytest.mark.parametrize("S,K", [(S, K) for S in (2, 10, 32) for K in (1, 3, 4)])
def test_step_and_eval_kernels_against_the_restatement(S, K, hip):
    from test_storage_gpu import random_storage_controller
    n_pre, n_main = 4099, 1543                                              # no multiples of 64
    sc = random_storage_controller(11 * S + K, hip, S=S, degree=K - 1, n_pre=n_pre, n_main=n_main)
    sc.materialize = True
    assert sc.regression_function.get_degree() == K
    sc.run_simulation()
    p, st, meta = sc.products[0], sc._storage_handle(0), sc._storage_meta[0]
    rng = np.random.default_rng(1000 * S + K)
    n_atoms = len(sc.book_plan.atoms)
    h_datoms = rng.normal(0.0, 0.3, (n_atoms, 5, NP))
    h_datoms[:, 3:] *= 0.1                                                  # (tangents of the exponent's coefficients)
    datoms = hip.from_numpy(h_datoms)
    h_coeffs = hip.book_get_coeffs(sc.book)
    coeffs = hip.from_numpy(h_coeffs)
    prod_coeffs = p.regression_coeffs.numpy()
    rs_p = StorageRestatement(p, K, True)
    rs = T.StorageTangentRestatement(p, K, True)
    n_dates = len(rs.dates)

    # -- backward step
    c = step_setup(sc, hip, rng, h_datoms, datoms, coeffs, S, K, n_pre)
    for roll, reg, flags in ((n_dates // 2, n_dates // 2 - 1, _abi.LSM_F32_CACHE), (n_dates // 2, n_dates // 2 - 1, 0),
                             (n_dates - 1, n_dates - 2, _abi.LSM_F32_CACHE), (-1, n_dates // 2, 0)):
        check_step(c, roll, reg, flags)

    # -- main simulation
    paths = sc.last_state["paths"].contiguous()
    h_paths = paths.cpu().numpy()
    h_dpaths = rng.normal(0.0, 0.2, (NP,) + h_paths.shape)
    dpaths = hip.from_numpy(h_dpaths)
    h_dcoeffs = rng.normal(0.0, 1.0, (len(h_coeffs), NP)) * np.abs(h_coeffs)[:, None]
    dcoeffs = hip.from_numpy(h_dcoeffs)
    plan = sc.book_plan
    E = max(plan.n_expo_rows, 1)
    cfs, expo = hip.zeros(1 + NP, plan.n_netting_sets, n_main), hip.zeros(1 + NP, plan.n_netting_sets, E, n_main)
    ops = sc._storage_ops(0)
    hip.tangent_storage_eval(sc.book, st, ops, datoms, coeffs, dcoeffs, paths, dpaths, cfs, expo)
    cfs0, expo0 = hip.zeros(plan.n_netting_sets, n_main), hip.zeros(plan.n_netting_sets, E, n_main)
    hip.storage_eval(sc.book, st, ops, paths, cfs0, expo0)
    hip.synchronize()
    assert np.array_equal(cfs[0].cpu().numpy(), cfs0.cpu().numpy()) and np.array_equal(expo[0].cpu().numpy(), expo0.cpu().numpy())
    expo_times = [float(t) for t in sc.exposure_timeline]
    by_time = {}
    for j, t in enumerate(rs.dates):
        by_time[t] = meta["action"][j]
    for i, t in enumerate(expo_times):
        by_time.setdefault(t, meta["expo"][i])
    atom = lambda q: atom_dual(sc, h_paths, h_dpaths, h_datoms, q)[:2]
    spot_at, num_at = (lambda t: atom(by_time[float(t)][1])), (lambda t: atom(by_time[float(t)][0]))
    blk = lambda a, off: a[off:off + S * K]
    offs = [sc._expo_coeff_base[0] + i * S * K for i in range(len(expo_times))]
    expo_c = np.stack([blk(h_coeffs, o).reshape(S, K) for o in offs])
    expo_dc = np.stack([np.stack([blk(h_dcoeffs[:, q], o).reshape(S, K) for o in offs]) for q in range(NP)])
    want_cf, want_dcf, want_e, want_de = rs.forward(expo_times, True, spot_at, num_at, prod_coeffs, expo_c, expo_dc)
    _c, _e, margin = rs_p.forward(expo_times, True, lambda t: spot_at(t)[0], lambda t: num_at(t)[0], prod_coeffs, expo_c)
    keep = margin >= MARGIN
    assert 1.0 - keep.mean() <= MAX_LEFT_OUT
    got_dcf, got_de = cfs[1:, 0].cpu().numpy(), expo[1:, 0].cpu().numpy()
    for got, want, tag in ((got_dcf, want_dcf, "cashflow"), (got_de[:, :len(expo_times)], want_de, "exposure")):
        big = np.abs(want).max()
        err = np.abs(got - want)[..., keep].max()
        print(S, K, tag, "tangent error / largest", err / big)
        assert err <= 1e-10 * big, (S, K, tag, err, big)
    assert np.allclose(cfs[0, 0].cpu().numpy()[keep], want_cf[keep], rtol=1e-10, atol=1e-12)


# ---- 3. Schwartz two-factor dual paths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["storage_const", "storage_short_last"])          # ANALYTICAL, EULER
def test_s2f_dual_paths_against_complex_step(name, hip):
    from mcx import aad
    sc = controller(name, hip, False)
    sc.run_simulation()
    sim, plan = sc._sim, sc.sim_plan
    g = storage_cases.load_golden(name)
    z = g["z_main"]
    d_z = hip.from_numpy(np.ascontiguousarray(np.transpose(z, (0, 2, 1))))
    n = z.shape[1]
    cs = T.ComplexStep(sc, plan, z)
    P = cs.P
    _, dd = aad.descriptor_tangents(sc, sc.model, False, mode="complex")      # the driver's descriptor tangents, [...][P]
    primal = hip.generate_paths(sim, 43, 0, n, inject_z=d_z).cpu().numpy()
    assert np.allclose(primal, cs.paths, rtol=1e-11, atol=1e-13)
    for c0 in range(0, P, NP):
        sel = list(range(c0, min(c0 + NP, P)))
        pad = lambda a: aad.pad_chunk(a, sel)
        paths, dpaths = hip.tangent_paths_s2f(sim, pad(dd["slots"]), pad(dd["init"]), pad(dd["aux"]), pad(dd["chol"]), 43, 0, n, d_z)
        assert np.array_equal(paths.cpu().numpy(), primal), (name, "the primal image is mcx_generate_paths'")
        got = dpaths.cpu().numpy()
        for q, j in enumerate(sel):
            want = cs.dpaths[j]
            big = np.abs(want).max()
            print(name, "parameter", j, "path tangent error / largest", np.abs(got[q] - want).max() / max(big, 1e-300))
            assert np.allclose(got[q], want, rtol=1e-11, atol=1e-13 * max(big, 1.0)), (name, j, np.abs(got[q] - want).max(), big)
        assert not got[len(sel):].any()


# ---- 4. additivity ---------------------------------------------------------------------------------------------------------------------
def test_pv_gradients_are_additive_over_the_products_of_a_netting_set(hip):
    """storage_mixed on identical draws: grad PV{storage, call} - grad PV{storage} = grad PV{call}.  (PV is linear in the products;
    the collateral threshold of the set only enters the exposure metrics, which are not compared.)"""
    def variant(keep):
        def build(mod):
            ns, model, rm = storage_cases.storage_mixed(mod)
            mix = mod["NettingSet"](name="mix", products=[p for p in ns[0].products if keep(p)], counterparty_id="cp", threshold=0.5,
                                    margin_period_of_risk=0.125)
            return [mix, ns[1]], model, rm
        return build

    is_storage = lambda p: getattr(p, "is_storage", False)
    pv_grad = {}
    for tag, keep in (("both", lambda p: True), ("storage", is_storage), ("call", lambda p: not is_storage(p))):
        sc = controller("storage_mixed", hip, True, build=variant(keep))
        res = sc.run_simulation()
        m_pv = [m.get_name() for m in sc.risk_metrics.metrics].index("pv")
        pv_grad[tag] = gradients(res)[0][m_pv][0]
        assert sc.timings["tangent"] is True
    want, got = pv_grad["call"], pv_grad["both"] - pv_grad["storage"]
    scale = np.abs(pv_grad["both"]).max()
    print("additivity: max error / max|row|", np.abs(got - want).max() / scale)
    assert (np.abs(got - want) <= 1e-8 * np.abs(want) + 1e-10 * scale).all(), (got, want)


# ---- 5. emulated ranks -----------------------------------------------------------------------------------------------------------------
def test_storage_shift_gradients_on_three_emulated_ranks(hip):
    from emulated_ranks import run_ranks
    from mcx import _native

    def build(be):
        sc = controller("storage_shift", be, True, inject=False)
        sc.materialize = False
        return sc

    ref = gradients(build(hip).run_simulation())
    out, calls = run_ranks(3, lambda rank: build(_native.HipBackend(0)), lambda sc, rank: gradients(sc.run_simulation()))
    assert calls["all_reduce"] > 0
    for rank, got in enumerate(out):
        for ns_r, ns_g in zip(ref, got):
            for m_r, m_g in zip(ns_r, ns_g):
                scale = np.abs(m_r).max(axis=1, keepdims=True)
                print("rank", rank, "max gradient difference / max|row|", (np.abs(m_r - m_g) / np.maximum(scale, 1e-300)).max())
                assert np.allclose(m_r, m_g, rtol=1e-9, atol=1e-12), (rank, m_r, m_g)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_configurations_forward_mode_cannot_take_are_refused(hip):
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    from mcx.models.heston import HestonModel
    mod = storage_cases.mcx_classes()
    ns, _model, rm = storage_cases.storage_const(mod)
    heston = HestonModel(0.0, 30.0, 0.002, 0.3, -0.5, 1.5, 0.04, 0.04, asset_id="gas")
    sc = SimulationController(ns, heston, mod["RiskMetrics"]([mod["PVMetric"]()]), 256, 256, 2, SimulationScheme.EULER, True, backend=hip)
    with pytest.raises(NotImplementedError, match="storage policy"):
        sc.run_simulation()
    sc = controller("storage_const", hip, True)
    sc.forward_mode = False
    with pytest.raises(NotImplementedError, match="storage policy"):
        sc.run_simulation()
    sc = controller("storage_const", hip, True)
    sc.compute_higher_derivatives()
    with pytest.raises(NotImplementedError, match="storage policy"):
        sc.run_simulation()


# ---- 7. books without a storage ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["EULER", "ANALYTICAL"])
def test_s2f_book_without_a_storage_keeps_its_route(scheme, hip, monkeypatch):
    """the Schwartz two-factor dual paths exist for books that hold a storage: a European call alone on that model must neither
    reach mcx_tangent_paths_s2f nor finish in run_with_tangent_book (which it never could before), whatever route it takes"""
    import cases
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController

    def never(*a, **k):
        raise AssertionError("mcx_tangent_paths_s2f reached by a book without a storage")

    monkeypatch.setattr(hip, "tangent_paths_s2f", never, raising=True)
    ns, model, rm = cases.s2f_european()
    sc = SimulationController(ns, model, rm, 512, 0, 2, getattr(SimulationScheme, scheme), True, backend=hip)
    res = sc.run_simulation()
    assert "forward_mode_passes" not in sc.timings, sc.timings
    grad = np.array(res.derivatives[0][0][0], dtype=np.float64)
    assert grad.shape == (6,) and np.isfinite(grad).all() and np.abs(grad).max() > 0.0, grad
