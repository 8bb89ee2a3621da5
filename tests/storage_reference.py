"""Plain numpy restatement of the gas storage's dynamic programme (test helper, in the spirit of lsm_reference.py: no kernel
arithmetic shared, numpy.linalg.lstsq on the raw monomials) — the checker of Philox-mode GPU runs, for which no fixture exists.

It is fed with per-date arrays of spot and numeraire (resolved from a paths tensor by `AtomReader`) and a Storage product, and
restates controller.py:294-471 of the reference for that product:
  * `backward`: the Longstaff-Schwartz induction over the regression timeline (action dates and exposure dates), all paths
    rolled from the integer grid states, `float32_quirk` reproducing the reference's float32 step buffer;
  * `forward`: the walk of the realised real-valued state through the main simulation -> cashflows, exposures, and per path the
    smallest relative decision margin it met (gap between best and second-best action value over the largest |action value|;
    ties between two forms of the same action do not count, see SAME_ACTION)."""
import numpy as np

# two candidates whose next states (in grid units, relative to S - 1) and cash (relative to the largest |action value|) agree to this
# are one action: choosing either moves a path's cashflows by ~1e-12 relative, a hundredth of what the comparisons resolve
SAME_ACTION = 1e-12


class AtomReader:
    """values of the book's atoms on a paths array [T][D][n] (host copy): a + d x + b exp(c0 + c1 x), x = paths[t_idx][col]"""

    def __init__(self, sc, paths):
        self.sc, self.paths = sc, np.asarray(paths)
        from mcx.request_interface.request_types import AtomicRequest, AtomicRequestType
        self._req, self._type = AtomicRequest, AtomicRequestType

    def value(self, atom_id: int) -> np.ndarray:
        a = self.sc.book_plan.atoms[atom_id]
        x = self.paths[a["t_idx"], a["col"]] if a["col"] >= 0 else np.zeros(self.paths.shape[2])
        v = a["a"] + a["d"] * x
        return v + a["b"] * np.exp(a["c0"] + a["c1"] * x) if a["b"] != 0.0 else v

    def spot(self, asset, t):
        return self.value(self.sc._comp.atom(self._req(self._type.SPOT), asset, float(t)))

    def numeraire(self, t):
        return self.value(self.sc._comp.atom(self._req(self._type.NUMERAIRE, float(t)), "numeraire", float(t)))


def _rate(points, v):
    """piecewise-linear rate curve on an array of volumes: flat outside the knots, left rate at a doubled knot"""
    xp, fp = np.array([p.point for p in points]), np.array([p.rate for p in points])
    if len(xp) == 1:
        return np.full_like(v, fp[0])
    left = np.clip(np.searchsorted(xp, v, side="left") - 1, 0, len(xp) - 2)
    x0, x1, y0, y1 = xp[left], xp[left + 1], fp[left], fp[left + 1]
    close = np.isclose(x0, x1)
    w = np.where(close, 0.0, (v - x0) / np.where(close, 1.0, x1 - x0))
    out = y0 + w * (y1 - y0)
    out = np.where(v <= xp[0], fp[0], out)
    return np.where(v >= xp[-1], fp[-1], out)


def _lerp(values, state):
    """values [n][S] interpolated at real states [n][B] (clamped to the grid)"""
    S = values.shape[1]
    b = np.clip(state, 0.0, S - 1.0)
    lo, hi = np.floor(b).astype(np.int64), np.ceil(b).astype(np.int64)
    v_lo, v_hi = np.take_along_axis(values, lo, axis=1), np.take_along_axis(values, hi, axis=1)
    return v_lo + (b - lo) * (v_hi - v_lo)


def _basis(x, K):
    return np.stack([x ** k for k in range(K)], axis=1)


class StorageRestatement:
    def __init__(self, product, K: int, float32_quirk: bool = True, centred: bool = False):
        """centred: solve the least squares on the monomials of z = (x - mid) / half-range and expand to powers of x in long
        double — algebraically the same regression, far better conditioned than the raw monomials of x ~ 30 that the reference
        (and centred=False) hands to lstsq.  The difference between the two is the restatement's OWN error in a coefficient
        or an exposure: raw monomials of degree 4 lose ~6 digits in the exposures."""
        self.p, self.K, self.f32, self.centred = product, K, float32_quirk, centred
        self.S = product.get_num_states()
        self.dates = [float(t) for t in product.product_timeline]
        self.next_dates = [float(t) for t in product.next_action_dates]

    # ---- one action date for states [n][B] -----------------------------------------------------------------------
    def step(self, j: int, state, spot, numeraire, coeffs):
        """-> (next state [n][B], cash / numeraire [n][B], relative decision margin [n][B] (inf on exact ties))"""
        p, cfg, S = self.p, self.p.storage_config, self.S
        t, nxt = self.dates[j], self.next_dates[j]
        w, nw = cfg.get_volume_constraint(t), cfg.get_volume_constraint(nxt)
        step = 0.0 if np.isclose(w.vmin, w.vmax, rtol=0.0, atol=1e-12) else (w.vmax - w.vmin) / (S - 1.0)
        scale = 0.0 if np.isclose(nw.vmin, nw.vmax, rtol=0.0, atol=1e-12) else (S - 1.0) / (nw.vmax - nw.vmin)
        period = max(nxt - t, 0.0)
        v = w.vmin + state * step
        nv = np.stack([np.minimum(v + _rate(cfg.get_injection_flexibility_slice(t), v) * period, nw.vmax),
                       np.clip(v, nw.vmin, nw.vmax),
                       np.maximum(v - _rate(cfg.get_withdrawal_flexibility_slice(t), v) * period, nw.vmin)], axis=2)      # [n][B][3]
        ns = np.zeros_like(nv) if scale == 0.0 else (nv - nw.vmin) * scale
        dv = nv - v[:, :, None]
        buy, sell = (spot + cfg.get_variable_injection_cost(t))[:, None], (spot - cfg.get_variable_withdrawal_cost(t))[:, None]
        price = np.stack([np.broadcast_to(buy, v.shape), np.where(dv[:, :, 1] >= 0.0, buy, sell), np.broadcast_to(sell, v.shape)], axis=2)
        cash = -dv * price
        value = cash.copy()
        if not nxt >= p.end_date - 1e-12:
            grid = _basis(spot, self.K) @ coeffs.T                                    # [n][S]
            for a in range(3):
                value[:, :, a] += _lerp(grid, ns[:, :, a])
        best = np.argmax(value, axis=2)[:, :, None]                                    # the first maximum
        order = np.argsort(-value, axis=2, kind="stable")
        top, second = order[:, :, :1], order[:, :, 1:2]
        at = lambda m, k: np.take_along_axis(m, k, axis=2)[:, :, 0]
        big = np.maximum(np.abs(value).max(axis=2), 1e-300)
        gap = at(value, top) - at(value, second)
        # the same action twice: a full (empty) store injects (withdraws) into the boundary it already sits on.  Exactly equal, or
        # equal up to the rounding of vmin + state * step against the boundary: either way the two lead to the same state and cash
        same = (np.abs(at(ns, top) - at(ns, second)) <= SAME_ACTION * (S - 1.0)) & (np.abs(at(cash, top) - at(cash, second)) <= SAME_ACTION * big)
        gap3 = at(value, top) - at(value, order[:, :, 2:3])                             # ... then the third action is the runner-up
        margin = np.where((gap == 0.0) | same, np.where(gap3 == 0.0, np.inf, gap3 / big), gap / big)
        pick = lambda m: np.take_along_axis(m, best, axis=2)[:, :, 0]
        return pick(ns), pick(cash) / numeraire[:, None], margin

    # ---- pre-simulation ------------------------------------------------------------------------------------------
    def backward(self, exposure_times, spot_at, numeraire_at):
        """-> {t_reg: dict(coeffs [S][K], Y [S][n], x [n])} for every regression date the reference visits (controller.py:294-383)"""
        pt = np.array(self.dates)
        reg_tl = sorted(set(self.dates) | {float(t) for t in exposure_times})
        n = len(spot_at(reg_tl[0]))
        coeffs_of_date = np.zeros((len(pt), self.S, self.K))
        last = len(pt)
        cache = {last: np.zeros((n, self.S))}
        out = {}
        for t_reg in reversed(reg_tl):
            idx = int(np.searchsorted(pt, t_reg))
            if idx >= len(pt):
                continue
            t_next = idx + 1 if pt[idx] == t_reg else idx
            if t_next < last:
                state = np.tile(np.arange(self.S, dtype=np.float64), (n, 1))
                step_value = np.zeros((n, self.S), dtype=np.float32 if self.f32 else np.float64)
                for j in range(t_next, last):
                    state, cf, _ = self.step(j, state, spot_at(pt[j]), numeraire_at(pt[j]), coeffs_of_date[j])
                    step_value += cf.astype(step_value.dtype)
                cache[t_next] = step_value.astype(np.float64) + _lerp(cache[last], state)
                last = t_next
            total = cache[t_next]
            x = spot_at(t_reg)
            Y = numeraire_at(t_reg)[:, None] * total
            sol = self._solve(x, Y)                                                     # [S][K]
            if pt[idx] == t_reg:
                coeffs_of_date[idx] = sol
            out[t_reg] = dict(coeffs=sol, Y=Y.T.copy(), x=x)
        return out

    def _solve(self, x, Y):
        K = self.K
        if not self.centred or not x.max() > x.min():
            return np.linalg.lstsq(_basis(x, K), Y, rcond=None)[0].T
        mid, half = 0.5 * (x.min() + x.max()), 0.5 * (x.max() - x.min())
        b = np.linalg.lstsq(_basis((x - mid) / half, K), Y, rcond=None)[0].T.astype(np.longdouble)      # [S][K] in powers of z
        raw = np.zeros_like(b)
        from math import comb
        for k in range(K):                                                           # z^k = sum_j C(k, j) x^j (-mid)^(k-j) / half^k
            for j in range(k + 1):
                raw[:, j] += b[:, k] * comb(k, j) * np.longdouble(-mid) ** (k - j) / np.longdouble(half) ** k
        return raw.astype(np.float64)

    # ---- main simulation -----------------------------------------------------------------------------------------
    def forward(self, exposure_times, want_cfs, spot_at, numeraire_at, prod_coeffs, expo_coeffs):
        """-> (cfs [n], exposures [E][n], smallest relative decision margin per path [n])"""
        pt = self.dates
        n = len(spot_at(pt[0]))
        state, cfs, margin = np.zeros((n, 1)), np.zeros(n), np.full(n, np.inf)
        j, expo = 0, []

        def act(j):
            nonlocal state, cfs, margin
            state, cf, m = self.step(j, state, spot_at(pt[j]), numeraire_at(pt[j]), prod_coeffs[j])
            cfs = cfs + cf[:, 0]
            margin = np.minimum(margin, m[:, 0])

        for i, t in enumerate(float(t) for t in exposure_times):
            while j < len(pt) and pt[j] <= t:
                act(j)
                j += 1
            grid = _basis(spot_at(t), self.K) @ expo_coeffs[i].T
            expo.append(_lerp(grid, state)[:, 0] / numeraire_at(t))
        if want_cfs or len(exposure_times) == 0:
            while j < len(pt):
                act(j)
                j += 1
        return cfs, (np.stack(expo) if expo else np.zeros((0, n))), margin
