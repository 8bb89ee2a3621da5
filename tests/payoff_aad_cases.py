"""Sensitivities of the payoff forms (binary, barrier with and without Brownian bridge, geometric basket / Asian, arithmetic basket
with the geometric control variate): the cases behind tests/golden/payoff_*_aad.npz, recorded from the reference's autograd by
tests/golden/gen_payoff_aad_golden.py.  `lib` is the namespace the classes are taken from: tests/cases.py (mcx) by default, the
reference's own classes when the generator records the fixtures.  Also the host pieces the tests of these cases share: the dual
paths of Black-Scholes slots by complex step, and a fixture's gradients through the numpy restatement of the dual forms."""
import copy

import numpy as np


def _lib(lib):
    if lib is None:
        import cases as lib
    return lib


def _sets(lib, prods):
    for k, p in enumerate(prods):
        p.name = f"p{k}"
    return [lib.NettingSet(name=p.name, products=[p]) for p in prods]


def binary(lib=None):
    lib = _lib(lib)
    model = lib.BlackScholesModel(0, 100.0, 0.03, 0.25)
    prods = [lib.BinaryOption(1.0, 100.5, 10.0, lib.OptionType.CALL), lib.BinaryOption(0.75, 99.0, 5.0, lib.OptionType.PUT)]
    return _sets(lib, prods), model, lib.RiskMetrics([lib.PVMetric()])


def barriers(lib=None, bridge=False):
    """the four barrier types, one of them with a second barrier, 4 to 6 monitoring dates, calls and puts"""
    lib = _lib(lib)
    model = lib.BlackScholesModel(0, 100.0, 0.03, 0.25)
    B, O = lib.BarrierOptionType, lib.OptionType
    prods = [lib.BarrierOption(0.0, 1.0, 100.0, 6, O.CALL, 125.0, B.UPANDOUT),
             lib.BarrierOption(0.0, 1.0, 105.0, 5, O.PUT, 90.0, B.DOWNANDIN),
             lib.BarrierOption(0.2, 1.2, 95.0, 5, O.CALL, 85.0, B.DOWNANDOUT, 130.0, B.UPANDOUT),
             lib.BarrierOption(0.0, 0.8, 100.0, 4, O.PUT, 110.0, B.UPANDIN)]
    if bridge:
        for p in prods:
            p.set_use_brownian_bridge()
    return _sets(lib, prods), model, lib.RiskMetrics([lib.PVMetric()])


def barriers_bridge(lib=None):
    return barriers(lib, bridge=True)


def basket_cv(lib=None):
    """the reference script's pair on three correlated assets: arithmetic call with the geometric control variate, geometric put"""
    lib = _lib(lib)
    ids = ["a1", "a2", "a3"]
    model = lib.BlackScholesMulti(0.0, 0.02, ids, [100, 105, 95], [0.4, 0.3, 0.25], [[1, .5, -.2], [.5, 1, .3], [-.2, .3, 1]])
    T = lib.BasketOptionType
    prods = [lib.BasketOption(1.0, ids, [.5, .3, .2], 100, lib.OptionType.CALL, T.ARITHMETIC, True),
             lib.BasketOption(1.0, ids, [.25, .25, .5], 97, lib.OptionType.PUT, T.GEOMETRIC)]
    return _sets(lib, prods), model, lib.RiskMetrics([lib.PVMetric()])


def geo_asian(lib=None):
    lib = _lib(lib)
    model = lib.BlackScholesModel(0, 100.0, 0.03, 0.25)
    prods = [lib.AsianOption(0.0, 1.0, 100.0, 5, lib.OptionType.CALL, lib.AsianAveragingType.GEOMETRIC)]
    return _sets(lib, prods), model, lib.RiskMetrics([lib.PVMetric()])


def exposure_book(lib=None):
    """binary + barrier + plain European in one netting set, PV and EPE on three dates through a pre-simulation"""
    lib = _lib(lib)
    model = lib.BlackScholesModel(0, 100.0, 0.03, 0.25)
    O = lib.OptionType
    prods = [lib.BinaryOption(1.0, 100.5, 10.0, O.CALL), lib.BarrierOption(0.0, 1.0, 100.0, 5, O.CALL, 125.0, lib.BarrierOptionType.UPANDOUT),
             lib.EuropeanOption(lib.Equity(), 1.0, 95.0, O.PUT)]
    for k, p in enumerate(prods):
        p.name = f"p{k}"
    ns = [lib.NettingSet(name="book", products=prods)]
    return ns, model, lib.RiskMetrics([lib.PVMetric(), lib.EPEMetric()], exposure_timeline=np.array([0.0, 0.5, 1.0]))


# name -> (builder, n_pre, n_main, num_steps, scheme name)
CASES = {
    "payoff_binary_euler_aad": (binary, 0, 1024, 3, "EULER"),
    "payoff_binary_analytical_aad": (binary, 0, 1024, 2, "ANALYTICAL"),
    "payoff_barrier_aad": (barriers, 0, 1024, 2, "ANALYTICAL"),
    "payoff_barrier_bridge_aad": (barriers_bridge, 0, 1024, 2, "ANALYTICAL"),
    "payoff_basket_cv_aad": (basket_cv, 0, 1024, 2, "ANALYTICAL"),
    "payoff_geo_asian_aad": (geo_asian, 0, 1024, 2, "EULER"),
    "payoff_exposure_aad": (exposure_book, 2048, 1024, 1, "ANALYTICAL"),
}
PV_ONLY = [k for k, v in CASES.items() if v[1] == 0]


def bridge_rows(g):
    """{product index: uniforms [2 * n_intervals][N]} from a fixture's recorded numpy blocks bridge_u_<product> [calls][N][intervals]"""
    out = {}
    for k in [k for k in g.files if k.startswith("bridge_u_")]:
        calls = g[k]
        rows = np.zeros((2 * calls.shape[2], calls.shape[1]))
        for bi in range(calls.shape[0]):
            rows[bi::2] = calls[bi].T
        out[int(k.rsplit("_", 1)[1])] = rows
    return out


def make_controller(name, backend, inject=True, tangent_payoffs=False, g=None, differentiate=True):
    """the controller of `name`; with inject, on the draws the reference consumed (g: the fixture, loaded when None)"""
    import cases
    build, n_pre, n_main, steps, scheme = CASES[name]
    ns, model, rm = build()
    sc = cases.SimulationController(ns, model, rm, n_main, n_pre, steps, getattr(cases.SimulationScheme, scheme), differentiate=differentiate,
                                    backend=backend)
    sc.materialize = True
    sc.tangent_payoffs = tangent_payoffs
    if inject:
        g = cases.load_golden(name) if g is None else g
        for key, which in (("z_main", "main"), ("z_pre", "pre")):
            if key in g.files:
                sc._inject[which] = (backend.from_numpy(np.ascontiguousarray(np.transpose(g[key], (0, 2, 1)))), None)      # [S][n_z][N]
        rows = bridge_rows(g)
        if rows:
            sc._inject["bridge_main"] = {p_i: backend.from_numpy(r) for p_i, r in rows.items()}
    return sc, g


# ---- the host side of a PV fixture: dual paths by complex step, gradients through the restatement --------------------------------
def complex_paths(model, plan, z, j, h):
    """paths [T][D][n] of Black-Scholes slots at theta_j + i h (complex float64 numpy) on the normals z [n_steps][n_z][n]: EULER
    (black_scholes.py:79-85) with the plan's correlation factor, ANALYTICAL (:61-67) with the models' closed-form factor"""
    from mcx import _abi, aad
    m = copy.deepcopy(model)
    aad._set_complex_step(m, j, h)
    slots = m._slots()
    assert all(sp.kind == _abi.MODEL_BS for sp in slots)
    n = z.shape[2]
    state = np.repeat(np.array(m._initial_state(), dtype=np.complex128)[:, None], n, axis=1)
    out = np.zeros((plan.n_dates, plan.n_state, n), dtype=np.complex128)
    for t in range(plan.n_initial_store):
        out[t] = state
    analytic = plan.scheme.name == "ANALYTICAL"
    chol = np.array([m._analytic_factor_entries(dt) for dt in plan.chol_dt], dtype=np.complex128).reshape(plan.chol.shape) if analytic \
        else plan.chol.astype(np.complex128)
    for k in range(plan.n_steps):
        st = plan.steps[k]
        zc = chol[st["chol_idx"]] @ z[k]
        aux = m._step_aux(plan.scheme, float(st["t1"]), float(st["dt"]))
        for s, sp in enumerate(slots):
            _s0, sigma, rate = sp.params[:3]
            if analytic:
                state[s] = state[s] * np.exp(aux[s][0] + (zc[s] - aux[s][1]))
            else:
                state[s] = state[s] + (rate * state[s] * st["dt"] + sigma * state[s] * (st["sqrt_dt"] * zc[s]))
        if st["store_idx"] >= 0:
            out[st["store_idx"]] = state
    return out


def restated_gradients(sc, g, dtype=np.float64):
    """(PV [n_ns], d PV / d theta [n_ns][P]) of a PV-only fixture through the numpy restatement of the dual forms: `sc` a compiled
    controller of the case (it ran once on any backend), paths and their tangents by complex step on the fixture's normals, atom and
    payoff-number tangents from the driver's own host functions"""
    from mcx import aad
    from payoff_tangent_reference import PayoffRestatement
    model, plan = sc.model, sc.sim_plan
    z = np.ascontiguousarray(np.transpose(g["z_main"], (0, 2, 1)))
    theta = [float(p.detach()) for p in model.get_model_params()]
    cols = [complex_paths(model, plan, z, j, 1e-30 * max(abs(th), 1e-2)) for j, th in enumerate(theta)]
    paths = cols[0].real
    dpaths = np.stack([c.imag / (1e-30 * max(abs(th), 1e-2)) for c, th in zip(cols, theta)])
    _d0, dd = aad.descriptor_tangents(sc, model, False)
    rs = PayoffRestatement(sc.book_plan, paths, dpaths, dd["atoms"], aad.payoff_tangents(sc, model), bridge_rows(g), dtype=dtype)
    img = rs.cashflows()
    return img[0].mean(axis=-1), img[1:].mean(axis=-1).T, rs


def restated_exposure_gradients(sc, g):
    """a fixture with a pre-simulation end to end on the host -> (results, derivatives) shaped [ns][metric][eval] for PV and EPE
    metrics: dual pre-simulation paths by complex step on z_pre, the dual normal equations of every (product, date) from the
    restatement (the cash-event copies [cf_begin, cf_end), the float32 value cache of the reference), the driver's host solve
    (aad._solve_dual on the centring of regression_centering), then main paths on z_main, dual cashflows, dual polynomial and
    analytic exposures, and the mean of 1[u > 0] du per exposure date"""
    from mcx import aad
    from mcx.metrics.metric import MetricType
    from payoff_tangent_reference import PayoffRestatement
    model, plan, bp = sc.model, sc.sim_plan, sc.book_plan
    theta = [float(p.detach()) for p in model.get_model_params()]
    P, K = len(theta), bp.n_basis
    hs = [1e-30 * max(abs(th), 1e-2) for th in theta]

    def dual_paths(key):
        z = np.ascontiguousarray(np.transpose(g[key], (0, 2, 1)))
        cols = [complex_paths(model, plan, z, j, h) for j, h in enumerate(hs)]
        return cols[0].real, np.stack([c.imag / h for c, h in zip(cols, hs)])

    _d0, dd = aad.descriptor_tangents(sc, model, False)
    dpay = aad.payoff_tangents(sc, model)
    pre = PayoffRestatement(bp, *dual_paths("z_pre"), dd["atoms"], dpay)
    lsm_plan, _ = sc._regression_plan()
    x_ids = sorted({x for _, _, _, atoms in lsm_plan for _, x in atoms})
    x_range = {x: (float(pre.atom(x).v.min()), float(pre.atom(x).v.max())) for x in x_ids}
    table, keep = aad.stateless_lsm_jobs(lsm_plan, x_range, sc._expo_coeff_base, K)
    coeffs, dcoeffs = np.zeros(max(len(bp.coeffs), 1)), np.zeros((max(len(bp.coeffs), 1), P))
    for q, (o, degenerate) in zip(table, keep):
        mom = pre.moments(int(q["product"]), int(q["first_event"]), int(q["num_atom"]), int(q["x_atom"]), float(q["shift"]), float(q["scale"]), K,
                          f32_cache=True)
        coeffs[o:o + K], dc = aad._solve_dual(mom, K, float(q["shift"]), float(q["scale"]), degenerate, P)
        dcoeffs[o:o + K] = dc.T
    main = PayoffRestatement(bp, *dual_paths("z_main"), dd["atoms"], dpay, bridge_rows(g))
    cfs, expo = main.cashflows(), main.exposures(coeffs, dcoeffs, aad._bs_exposure_slots(sc, sc, list(range(P))))
    rows = sc.metric_exposure_indices.numpy().astype(int)
    results, grads = [], []
    for ns_i in range(cfs.shape[1]):
        rv, gv = [], []
        for m in sc.risk_metrics.metrics:
            if m.metric_type == MetricType.PV:
                rv.append([(cfs[0, ns_i].mean(), 0.0)])
                gv.append([tuple(cfs[1:, ns_i].mean(axis=-1))])
            else:
                assert m.metric_type == MetricType.EPE
                u, du = expo[0, ns_i][rows], expo[1:, ns_i][:, rows]                           # [dates][n], [P][dates][n]
                rv.append([(np.maximum(u[e], 0.0).mean(), 0.0) for e in range(len(rows))])
                gv.append([tuple(np.where(u[e] > 0.0, du[:, e], 0.0).mean(axis=-1)) for e in range(len(rows))])
        results.append(rv)
        grads.append(gv)
    return results, grads, (pre, main, len(table))


# ---- kernel-level books: every payoff form the dual kernels have, on host-made inputs ---------------------------------------------
def _bs():
    import cases
    return cases.BlackScholesModel(0, 100.0, 0.03, 0.25)


def _all_barriers(n_obs):
    """every barrier type x call / put with n_obs monitored dates"""
    import cases
    B, O = cases.BarrierOptionType, cases.OptionType
    level = {B.UPANDOUT: 118.0, B.DOWNANDOUT: 86.0, B.UPANDIN: 112.0, B.DOWNANDIN: 92.0}
    return [cases.BarrierOption(0.0, 1.0, 100.0 if o == O.CALL else 103.0, n_obs, o, level[b], b) for b in level for o in (O.CALL, O.PUT)]


def _kernel_products(name):
    import cases
    B, O, T = cases.BarrierOptionType, cases.OptionType, cases.BasketOptionType
    if name == "binary":
        return _bs(), [cases.BinaryOption(1.0, 100.5, 10.0, O.CALL), cases.BinaryOption(0.75, 99.0, 5.0, O.PUT)]
    if name in ("barrier2", "barrier6"):
        return _bs(), _all_barriers(int(name[-1]))
    if name == "double":
        return _bs(), [cases.BarrierOption(0.2, 1.2, 95.0, 5, O.CALL, 85.0, B.DOWNANDOUT, 130.0, B.UPANDOUT),
                       cases.BarrierOption(0.0, 1.0, 102.0, 4, O.PUT, 120.0, B.UPANDIN, 80.0, B.DOWNANDOUT)]
    if name == "bridge":
        prods = [cases.BarrierOption(0.0, 1.0, 100.0, 6, O.CALL, 125.0, B.UPANDOUT), cases.BarrierOption(0.0, 1.0, 105.0, 2, O.PUT, 90.0, B.DOWNANDIN),
                 cases.BarrierOption(0.2, 1.2, 95.0, 5, O.CALL, 85.0, B.DOWNANDOUT, 130.0, B.UPANDOUT),
                 cases.BarrierOption(0.0, 0.8, 100.0, 4, O.PUT, 110.0, B.UPANDIN, 80.0, B.DOWNANDOUT)]
        for p in prods:
            p.set_use_brownian_bridge()
        return _bs(), prods
    if name == "geo2":
        model = cases.BlackScholesMulti(0.0, 0.02, ["a1", "a2"], [100, 105], [0.4, 0.3], [[1, .5], [.5, 1]])
        return model, [cases.BasketOption(1.0, ["a1", "a2"], [.6, .4], 100, O.CALL, T.GEOMETRIC), cases.BasketOption(1.0, ["a1", "a2"], [.5, .5], 104, O.PUT, T.GEOMETRIC)]
    if name == "cv":
        ns, model, _ = basket_cv()
        return model, [n.products[0] for n in ns]
    if name == "asian":
        return _bs(), [cases.AsianOption(0.0, 1.0, 100.0, 5, O.CALL, cases.AsianAveragingType.GEOMETRIC),
                       cases.AsianOption(0.25, 1.25, 102.0, 4, O.PUT, cases.AsianAveragingType.GEOMETRIC)]
    if name == "plain":                                                        # no payoff mode at all: the old instantiation
        return _bs(), [cases.AsianOption(0.0, 1.0, 100.0, 5, O.CALL, cases.AsianAveragingType.ARITHMETIC),
                       cases.AsianOption(0.25, 1.25, 102.0, 4, O.PUT, cases.AsianAveragingType.ARITHMETIC)]
    raise KeyError(name)


KERNEL_BOOKS = ["binary", "barrier2", "barrier6", "double", "bridge", "geo2", "cv", "asian"]


def kernel_controller(name, backend, n=64, exposures=False):
    """a compiled controller of the kernel-level book `name`: all products in ONE netting set per product (PV), or — exposures — in
    one netting set with EPE on three dates, so that every product also has regression jobs"""
    import cases
    model, prods = _kernel_products(name)
    for k, p in enumerate(prods):
        p.name = f"k{k}"
    if exposures:
        ns, rm = [cases.NettingSet(name="book", products=prods)], cases.RiskMetrics([cases.PVMetric(), cases.EPEMetric()], exposure_timeline=np.array([0.0, 0.4, 0.8]))
    else:
        ns, rm = [cases.NettingSet(name=p.name, products=[p]) for p in prods], cases.RiskMetrics([cases.PVMetric()])
    sc = cases.SimulationController(ns, model, rm, n, n if exposures else 0, 1, cases.A, backend=backend)
    sc.materialize, sc.allow_fused = True, False
    sc.run_simulation()
    return sc


def kernel_inputs(plan, n_state, n_dates, n, seed, NP=4):
    """host-made inputs of the dual book kernels for `plan`: spots around the barrier levels and strikes, independent per date, with
    random tangents; atom, payoff-number and coefficient tangents; bridge uniforms per product"""
    rng = np.random.default_rng(seed)
    paths = 100.0 * np.exp(0.18 * rng.standard_normal((n_dates, n_state, n)))
    dpaths = rng.normal(0.0, 1.0, (NP, n_dates, n_state, n)) * paths[None] * 0.01
    datoms = rng.normal(0.0, 0.3, (len(plan.atoms), 5, NP))
    datoms[:, 3:] *= 0.1
    ev = plan.events
    dpayoff = np.zeros((len(ev), NP))
    for q in range(len(ev)):
        if ev["kind"][q] == 2 and ev["aux"][q][0] == 2.0:
            dpayoff[q] = rng.normal(0.0, 1.0, NP)
        if ev["kind"][q] == 2 and ev["aux"][q][0] == 5.0:
            dpayoff[q] = rng.normal(0.0, 1.0, NP) * abs(plan.coeffs[ev["coeff_off"][q]]) * 0.1
    bridge = {}
    for q in range(len(ev)):
        if ev["kind"][q] == 2 and ev["aux"][q][0] == 5.0:
            draw_id = int(plan.coeffs[ev["coeff_off"][q] + 1])
            n_int = int(ev["term_end"][q] - ev["term_begin"][q]) - 1
            if draw_id not in bridge:
                bridge[draw_id] = rng.uniform(0.0, 1.0, (2 * n_int, n))
    return dict(paths=paths, dpaths=dpaths, datoms=datoms, dpayoff=dpayoff, bridge=bridge)
