"""The reference's LSM pipeline for the two Heston fixture books, restated in numpy with explicit tangents (test helper; no torch,
nothing of the library's kernels or of its host solves): dual paths from tests/heston_tangent_reference.py, then — written from the
reference's controller (controller.py:296-383 regression, :385-471 evaluation) and products (european_option.py,
bermudan_option.py) — the backward induction with the float32 cashflow cache, the polynomial regression per date and state, the
exercise policy frozen as the tape freezes it (no gradient through `should_exercise`), exposures and cashflows of the main
simulation, and the metrics PV / EPE / ENE / PFE / EEPE per netting set.

The regression is solved from dual normal equations, G c = r => dc = G^-1 (dr - dG c), by Gaussian elimination in the working
dtype (np.float64 or np.longdouble), on the basis ((x - shift) scale)^k.  basis="centred": shift and scale map the pre-simulation's
range of x to [-1, 1]; basis="raw": the reference's own monomials x^k.  The fitted polynomial is the same function either way;
only the conditioning differs, which is what tests/test_tangent_heston_host.py measures."""
import types

import numpy as np

import heston_tangent_reference as hr
from heston_tangent_reference import Dual


def _exp(a):
    v = np.exp(a.v)
    return Dual(v, v * a.d)


def _f32(a):
    """the value through the reference's float32 cf_cache (controller.py:312-351); the gradient passes"""
    return Dual(a.v.astype(np.float32).astype(a.v.dtype), a.d)


def _solve(G, r):
    """Gaussian elimination with partial pivoting in the dtype of G (numpy's solvers stop at float64)"""
    G, r = G.copy(), r.copy()
    K = len(r)
    for c in range(K):
        p = c + int(np.argmax(np.abs(G[c:, c])))
        G[[c, p]], r[[c, p]] = G[[p, c]], r[[p, c]]
        for q in range(c + 1, K):
            f = G[q, c] / G[c, c]
            G[q, c:] -= f * G[c, c:]
            r[q] -= f * r[c]
    x = np.zeros_like(r)
    for c in reversed(range(K)):
        x[c] = (r[c] - G[c, c + 1:] @ x[c + 1:]) / G[c, c]
    return x


class Fit:
    """least-squares polynomial of degree K-1 of the dual y on the dual x, with dual coefficients; evaluates on other dual x"""

    def __init__(self, x, y, K, basis):
        T = x.v.dtype.type
        lo, hi = x.v.min(), x.v.max()
        self.degenerate = not (hi > lo)
        if self.degenerate:
            # every path has the same x (the calibration date): lstsq's minimum-norm solution predicts the mean of y at that x
            self.mean = (y.v.mean(), y.d.mean(axis=1))
            return
        self.shift, self.scale = (T(0.5) * (lo + hi), T(2.0) / (hi - lo)) if basis == "centred" else (T(0.0), T(1.0))
        z = (x - self.shift) * self.scale
        zp = [Dual.const(1.0, z)]
        for _ in range(2 * K - 2):
            zp.append(zp[-1] * z)
        idx = np.arange(K)[:, None] + np.arange(K)[None, :]
        m = np.array([p.v.sum() for p in zp])
        dm = np.array([p.d.sum(axis=1) for p in zp])                          # [2K-1][P]
        zy = [zp[k] * y for k in range(K)]
        r, dr = np.array([p.v.sum() for p in zy]), np.array([p.d.sum(axis=1) for p in zy])
        G = m[idx]
        self.c = _solve(G, r)
        self.dc = np.stack([_solve(G, dr[:, q] - dm[:, q][idx] @ self.c) for q in range(dm.shape[1])])      # [P][K]
        self.cond = float(np.linalg.cond(G.astype(np.float64)))

    def __call__(self, x):
        if self.degenerate:
            return Dual(np.full_like(x.v, self.mean[0]), np.repeat(self.mean[1][:, None], len(x.v), axis=1))
        z = (x - self.shift) * self.scale
        out, zp = None, Dual.const(1.0, z)
        for k in range(len(self.c)):
            ck = Dual(np.full_like(x.v, self.c[k]), np.repeat(self.dc[:, k][:, None], len(x.v), axis=1))
            out = ck * zp if out is None else out + ck * zp
            zp = zp * z
        return out


class Sim:
    """dual paths of one simulation with the closed forms the products ask of the model: spot and the deterministic numeraire"""

    def __init__(self, tb, timeline, rate, z, u, dtype):
        self.paths, self.dpaths, self.margins = hr.dual_paths(tb, z, u, dtype)
        self.timeline, self.dtype, self.n, self.P = np.asarray(timeline, dtype=np.float64), dtype, z.shape[2], self.dpaths.shape[0]
        self.rate = rate

    def _t(self, t):
        i = int(np.argmin(np.abs(self.timeline - t)))
        assert abs(self.timeline[i] - t) < 1e-12
        return i

    def spot(self, t):
        i = self._t(t)
        return _exp(Dual(self.paths[i, 0].copy(), self.dpaths[:, i, 0].copy()))

    def numeraire(self, t):
        """exp(rate (t - t0)), t0 = 0: a dual number in the rate, parameter 2 (heston.py:261-278 of the reference)"""
        T = self.dtype
        v = np.exp(T(self.rate) * T(t))
        d = np.zeros((self.P, self.n), dtype=T)
        d[2] = v * T(t)
        return Dual(np.full(self.n, v, dtype=T), d)

    def zero(self):
        return Dual(np.zeros(self.n, dtype=self.dtype), np.zeros((self.P, self.n), dtype=self.dtype))


def _payoff(spot, strike, sign):
    return hr.dclamp((spot - strike) * sign, 0.0)


def european(pre, main, expo_dates, maturity, strike, sign, K, basis):
    """-> (cashflows of the main simulation, [exposure per date], fits) of one European option (regression dates = the exposure
    dates)"""
    y_pre = _f32(_payoff(pre.spot(maturity), strike, sign) / pre.numeraire(maturity))
    expo, fits = [], []
    for t in expo_dates:
        if t >= maturity:                                                     # only cashflows strictly after t count (controller.py:323)
            expo.append(main.zero())
            continue
        fits.append(Fit(pre.spot(t), pre.numeraire(t) * y_pre, K, basis))
        expo.append(fits[-1](main.spot(t)) / main.numeraire(t))
    return _payoff(main.spot(maturity), strike, sign) / main.numeraire(maturity), expo, fits


def american(pre, main, expo_dates, dates, strike, sign, K, basis):
    """one exercise right on `dates`; state 1 = alive, state 0 = exercised (worth nothing, coefficients zero).  Backward induction
    on the pre-simulation: W_i = value after date i of an alive option along the policy, regressed at every date; the policy is the
    boolean immediate > continuation of the PRIMAL fits and carries no gradient.  -> (cashflows, [exposure per date], fits)"""
    n_d = len(dates)
    fits = [None] * n_d
    W = pre.zero()                                                            # after the last date: nothing
    for i in reversed(range(n_d)):
        if i < n_d - 1:
            j = i + 1                                                         # the one uncached date of this step (controller.py:333)
            imm = _payoff(pre.spot(dates[j]), strike, sign)
            cont = fits[j](pre.spot(dates[j])).v if j < n_d - 1 else np.zeros(pre.n, dtype=pre.dtype)
            ex = imm.v > cont
            cf = _f32(imm * ex.astype(pre.dtype) / pre.numeraire(dates[j]))
            W = _f32(cf + Dual(np.where(ex, 0.0, W.v).astype(pre.dtype), np.where(ex, 0.0, W.d).astype(pre.dtype)))
        fits[i] = Fit(pre.spot(dates[i]), pre.numeraire(dates[i]) * W, K, basis)
    alive = np.ones(main.n, dtype=bool)
    cfs, expo = main.zero(), {}
    for i, t in enumerate(dates):
        imm = _payoff(main.spot(t), strike, sign)
        cont = fits[i](main.spot(t)) if i < n_d - 1 else main.zero()
        ex = alive & (imm.v > cont.v)
        cfs = cfs + imm * ex.astype(main.dtype) / main.numeraire(t)
        alive = alive & ~ex
        if any(abs(t - e) < 1e-12 for e in expo_dates):                        # the exposure of the state reached at t
            c = fits[i](main.spot(t)) / main.numeraire(t)
            expo[round(float(t), 12)] = Dual(np.where(alive, c.v, 0.0), np.where(alive, c.d, 0.0))
    return cfs, [expo[round(float(t), 12)] for t in expo_dates], fits


def metrics(metric_list, cfs, expo, q_index):
    """results [metric][eval] of (value, 0.0) and derivatives [metric][eval] of a P-tuple for one netting set: cfs the netted dual
    cashflows, expo the netted dual exposure per date"""
    res, grad = [], []
    epe = [(np.maximum(u.v, 0).mean(), np.where(u.v > 0, u.d, 0).mean(axis=1)) for u in expo]
    for name, arg in metric_list:
        if name == "PV":
            rows = [(cfs.v.mean(), cfs.d.mean(axis=1))]
        elif name == "EPE":
            rows = epe
        elif name == "ENE":
            rows = [(np.minimum(u.v, 0).mean(), np.where(u.v < 0, u.d, 0).mean(axis=1)) for u in expo]
        elif name == "PFE":
            rows = []
            for u in expo:
                k = np.argsort(u.v, kind="stable")[q_index(arg)]
                rows.append((u.v[k], u.d[:, k]))
        elif name == "EEPE":
            rows = [(np.mean([v for v, _ in epe]), np.mean([d for _, d in epe], axis=0))]
        else:
            raise KeyError(name)
        res.append([(float(v), 0.0) for v, _ in rows])
        grad.append([tuple(float(x) for x in d) for _, d in rows])
    return res, grad


def run_fixture(name, g, dtype=np.float64, degree=None, basis="centred"):
    """the fixture `name` end to end on the host -> SimpleNamespace(results, derivatives, model_param_names, pre, main, fits)"""
    import cases
    import heston_aad_cases as hcases
    from mcx.plan import SimPlan
    build, n_pre, n_main, steps, scheme = hcases.CASES[name]
    ns, model, rm = build()
    model.perform_smoothing = True                                             # differentiate=True switches the smoothing on
    sc = cases.SimulationController(ns, model, rm, n_main, n_pre, steps, getattr(cases.SimulationScheme, scheme), differentiate=False,
                                    backend=types.SimpleNamespace(name="stub"))
    timeline = sc.simulation_timeline.numpy()
    plan = SimPlan(model, timeline, sc.simulation_scheme, steps)
    tb = hr.tables_of(plan, *hcases.bare_tables(model, plan, True), True)
    draws = hcases.injected_draws(g)
    rate = float(model.get_model_params()[2].detach())
    pre, main = (Sim(tb, timeline, rate, *draws[w], dtype) for w in ("pre", "main"))
    K = (hcases.REGRESSION_DEGREE.get(name, 2) if degree is None else degree) + 1
    expo_dates = [float(t) for t in rm.exposure_timeline] if hasattr(rm, "exposure_timeline") else [float(t) for t in sc.exposure_timeline]
    mets = [(m.metric_type.name, getattr(m, "quantile", None)) for m in rm.metrics]
    q_index = lambda q: int(np.ceil(np.float32(q * n_main))) - 1              # pfe_metric.py:59 of the reference, float32 as there
    results, derivatives, all_fits = [], [], []
    for netting_set in ns:
        cfs, expo = main.zero(), [main.zero() for _ in expo_dates]
        for p in netting_set.products:
            sign = 1.0 if p.option_type == cases.OptionType.CALL else -1.0
            strike = float(np.asarray(p.strike).reshape(-1)[0]) if hasattr(p, "strike") else float(p._K)
            dates = [float(t) for t in p.product_timeline]
            if p.get_num_states() > 1:
                c, e, fits = american(pre, main, expo_dates, dates, strike, sign, K, basis)
            else:
                c, e, fits = european(pre, main, expo_dates, dates[0], strike, sign, K, basis)
            all_fits += [f for f in fits if not f.degenerate]
            cfs = cfs + c
            expo = [a + b for a, b in zip(expo, e)]
        r, d = metrics(mets, cfs, expo, q_index)
        results.append(r)
        derivatives.append(d)
    return types.SimpleNamespace(results=results, derivatives=derivatives, model_param_names=model.get_model_param_names(), pre=pre, main=main,
                                 fits=all_fits)
