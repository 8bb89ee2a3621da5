"""Numpy restatement of the dual payoff forms of csrc/kt_book.hip (test helper; no kernel arithmetic shared): the option events of a
book plan in the aggregation modes 0-5 per path, value and NP tangents in explicit arrays.

The derivative is the one of the reference's tape: fuzzy indicators clamp((x + eps) / (2 eps), 0, 1) whose gradient passes on the
closed band (torch.clamp), torch.maximum(x, 0) with 1/2 at the tie, torch.max / torch.min over the monitored spots handing the
gradient to the FIRST extremal spot in monitoring order, bridge uniforms without tangent.  The one host-computed number of an event
(mode 2: the closed-form geometric price aux[1]; mode 5: the bridge constant parked at coeff_off) takes its tangent from the event's
row of `dpayoff`.

`dtype`: np.float64, or np.longdouble for the yardstick's own rounding (`rounding_gap`).  `margins` collects, per event, how close a
path comes to a band edge, a payoff kink or a tie among the monitored spots: there a device whose exp / log differ from numpy's by
ulps may take the other mask."""
import numpy as np

from mcx import _abi

EPS = 0.05                                    # maths.py:8, the default of compute_degree_of_truth


class Dual:
    """value v [n] and tangents d [NP][n]"""
    __slots__ = ("v", "d")

    def __init__(self, v, d):
        self.v, self.d = v, d

    @staticmethod
    def const(c, like):
        return Dual(np.full_like(like.v, c), np.zeros_like(like.d))

    @staticmethod
    def uniform(c, dc, n, dtype):
        """a number that is the same on every path: value c, tangents dc [NP]"""
        return Dual(np.full(n, c, dtype=dtype), np.repeat(np.asarray(dc, dtype=dtype)[:, None], n, axis=1))

    def __add__(self, o):
        return Dual(self.v + o.v, self.d + o.d) if isinstance(o, Dual) else Dual(self.v + o, self.d.copy())

    __radd__ = __add__

    def __sub__(self, o):
        return Dual(self.v - o.v, self.d - o.d) if isinstance(o, Dual) else Dual(self.v - o, self.d.copy())

    def __rsub__(self, c):
        return Dual(c - self.v, -self.d)

    def __mul__(self, o):
        if isinstance(o, Dual):
            return Dual(self.v * o.v, self.d * o.v + self.v * o.d)
        return Dual(self.v * o, self.d * o)

    __rmul__ = __mul__

    def __truediv__(self, o):
        if isinstance(o, Dual):
            v = self.v / o.v
            return Dual(v, (self.d - v * o.d) / o.v)
        return Dual(self.v / o, self.d / o)


def dexp(a):
    v = np.exp(a.v)
    return Dual(v, v * a.d)


def dlog(a):
    return Dual(np.log(a.v), a.d / a.v)


def dclamp01(a, margins=None, tag=None):
    """torch.clamp(a, 0, 1): the gradient passes iff 0 <= a <= 1"""
    if margins is not None:
        margins.setdefault(tag, []).append(np.minimum(np.abs(a.v), np.abs(a.v - 1.0)))
    mask = (a.v >= 0.0) & (a.v <= 1.0)
    return Dual(np.clip(a.v, 0.0, 1.0), np.where(mask, a.d, 0.0))


def dmax0(a, margins=None, tag=None):
    """torch.maximum(a, 0): gradient 1 above, 1/2 at the tie, 0 below"""
    if margins is not None:
        margins.setdefault(tag, []).append(np.abs(a.v))
    w = np.where(a.v > 0.0, 1.0, np.where(a.v == 0.0, 0.5, 0.0)).astype(a.v.dtype)
    return Dual(np.maximum(a.v, 0.0), w * a.d)


def fuzzy(x, margins=None, tag=None):
    """compute_degree_of_truth(x, True) with the default eps"""
    return dclamp01((x + EPS) / (2.0 * EPS), margins, tag)


class PayoffRestatement:
    """the events of `plan` (mcx.plan book plan: atoms, terms, events, products, coeffs) on paths [T][D][n] with tangents dpaths
    [NP][T][D][n], atom tangents datoms [n_atoms][5][NP] and payoff-number tangents dpayoff [n_events][NP] (None: zero).
    bridge: {draw id: uniforms [2 * n_intervals][n]} of the bridge events."""

    def __init__(self, plan, paths, dpaths, datoms, dpayoff=None, bridge=None, dtype=np.float64):
        self.plan, self.dtype = plan, dtype
        self.paths, self.dpaths = np.asarray(paths, dtype=dtype), np.asarray(dpaths, dtype=dtype)
        self.datoms = np.asarray(datoms, dtype=dtype)
        self.NP, self.n = self.dpaths.shape[0], self.paths.shape[2]
        self.dpayoff = np.zeros((len(plan.events), self.NP), dtype=dtype) if dpayoff is None else np.asarray(dpayoff, dtype=dtype)
        self.bridge = bridge or {}
        self.margins = {}
        self.hits = {}                        # bridge event -> [n] bool: some interval's fuzzy hit is non-zero on the path

    def atom(self, a_id):
        a, da = self.plan.atoms[a_id], self.datoms[a_id]
        uni = lambda k, name: Dual.uniform(self.dtype(a[name]), da[k], self.n, self.dtype)
        if a["col"] >= 0:
            x = Dual(self.paths[a["t_idx"], a["col"]].copy(), self.dpaths[:, a["t_idx"], a["col"]].copy())
        else:
            x = Dual.uniform(self.dtype(0.0), np.zeros(self.NP), self.n, self.dtype)
        v = uni(0, "a") + uni(1, "d") * x
        if a["b"] != 0.0:
            v = v + uni(2, "b") * dexp(uni(3, "c0") + uni(4, "c1") * x)
        return v

    def _terms(self, e):
        return [(self.dtype(self.plan.terms["w"][j]), self.atom(int(self.plan.terms["atom"][j]))) for j in range(e["term_begin"], e["term_end"])]

    def event(self, q):
        """normalised dual cashflow of cash event q (CASHFLOW without per-term denominators, OPTION in the modes 0-5)"""
        e = self.plan.events[q]
        m, tag = self.margins, f"event{q}"
        num = self.atom(int(e["num_atom"]))
        K, sign, aux = self.dtype(e["strike"]), self.dtype(e["sign"]), [self.dtype(x) for x in e["aux"]]
        assert all(self.plan.terms["den"][j] < 0 for j in range(e["term_begin"], e["term_end"]))
        if e["kind"] == _abi.EV_CASHFLOW:
            val = None
            for w, av in self._terms(e):
                val = av * w if val is None else val + av * w
            return val / num
        assert e["kind"] == _abi.EV_OPTION
        mode = int(e["aux"][0])
        if mode in (4, 5):
            return self._barrier(q, e, num, K, sign, aux)
        terms = self._terms(e)
        val = terms[0][1] * terms[0][0]
        for w, av in terms[1:]:
            val = val + av * w
        if mode == 0:
            return dmax0((val - K) * sign, m, tag + ":kink") / num
        if mode == 3:                                                                         # binary_option.py:38-43
            dot = dclamp01((val - K + aux[2]) / (2.0 * aux[2]), m, tag + ":band")
            return ((dot if sign > 0 else 1.0 - dot) * aux[1]) / num
        glog = None
        for w, av in terms:                                                                   # basket_option.py:62-65
            t = dlog(av + self.dtype(1e-10)) * w
            glog = t if glog is None else glog + t
        geo = dmax0((dexp(glog) - K) * sign, m, tag + ":kink")
        if mode == 1:
            return geo / num
        assert mode == 2                                                                      # basket_option.py:72-78
        imm = dmax0((val - K) * sign, m, tag + ":kink")
        return (imm - geo + Dual.uniform(aux[1], self.dpayoff[q], self.n, self.dtype)) / num

    def _barrier(self, q, e, num, K, sign, aux):
        m, tag = self.margins, f"event{q}"
        types = int(e["aux"][3])
        t1, t2 = types & 7, types >> 3
        spots = [av for _w, av in self._terms(e)]
        V = np.stack([s.v for s in spots])                                                    # [dates][n]
        if len(spots) > 1:
            srt = np.sort(V, axis=0)
            m.setdefault(tag + ":tie", []).append(np.minimum(srt[1] - srt[0], srt[-1] - srt[-2]) / np.abs(srt[-1]))
        rows = np.arange(self.n)
        pick = lambda idx: Dual(V[idx, rows], np.stack([s.d for s in spots])[idx, :, rows].T)
        mx, mn = pick(np.argmax(V, axis=0)), pick(np.argmin(V, axis=0))                       # numpy: the first extremal index
        x = self.atom(int(e["x_atom"]))
        pay = dmax0((x - K) * sign, m, tag + ":kink")

        def ind(t, level):
            below = fuzzy(level - mx, m, tag + ":band") if t in (1, 3) else fuzzy(mn - level, m, tag + ":band")
            return below if t <= 2 else 1.0 - below

        keep = [None, None]
        if int(e["aux"][0]) == 5:
            co = int(e["coeff_off"])
            c = Dual.uniform(self.dtype(self.plan.coeffs[co]), self.dpayoff[q], self.n, self.dtype)
            u = np.asarray(self.bridge[int(self.plan.coeffs[co + 1])], dtype=self.dtype)
            for bi, level in enumerate((aux[1], aux[2]) if t2 else (aux[1],)):
                logs = [dlog(s / level) for s in spots]
                k_ = Dual.const(1.0, spots[0])
                for k in range(len(spots) - 1):
                    p = dexp(c * (logs[k] * logs[k + 1]))
                    hit = fuzzy(p - u[2 * k + bi], m, tag + ":band")
                    self.hits[q] = self.hits.get(q, np.zeros(self.n, dtype=bool)) | (hit.v > 0.0)
                    k_ = k_ * (1.0 - hit)
                keep[bi] = k_
        pay = pay * ind(t1, aux[1])
        if keep[0] is not None:
            pay = pay * (keep[0] if t1 <= 2 else 1.0 - keep[0])
        if t2:
            pay = pay * ind(t2, aux[2])
            if keep[1] is not None:
                pay = pay * (keep[1] if t2 <= 2 else 1.0 - keep[1])
        return pay / num

    def cashflows(self):
        """[1 + NP][n_netting_sets][n]: the cash events among the main-pass events [ev_begin, ev_end) of every product summed per
        netting set (mcx_tangent_eval's d_cfs; the regression reads the product's second copy of them, [cf_begin, cf_end))"""
        pr = self.plan.products
        n_ns = int(pr["netting_set"].max()) + 1
        out = np.zeros((1 + self.NP, n_ns, self.n), dtype=self.dtype)
        for p in range(len(pr)):
            for q in range(pr["ev_begin"][p], pr["ev_end"][p]):
                if self.plan.events["kind"][q] > _abi.EV_OPTION:
                    continue
                v = self.event(q)
                out[0, pr["netting_set"][p]] += v.v
                out[1:, pr["netting_set"][p]] += v.d
        return out

    def exposures(self, coeffs, dcoeffs, ev_param=None):
        """[1 + NP][n_netting_sets][n_rows][n]: the exposure events of every product summed per netting set and row
        (mcx_tangent_eval's d_expo) — regressed polynomials sum_k c_k x^k / numeraire with dual coefficients coeffs [n_coeffs],
        dcoeffs [n_coeffs][NP], and the analytic Black-Scholes exposure (european_option.py:123-145) whose sigma / rate take the
        tangent slots ev_param [n_events][2] (-1: none)"""
        import math
        pr, ev, K = self.plan.products, self.plan.events, self.plan.n_basis
        n_ns, n_rows = int(pr["netting_set"].max()) + 1, max(int(self.plan.n_expo_rows), 1)
        out = np.zeros((1 + self.NP, n_ns, n_rows, self.n), dtype=self.dtype)
        erf = np.vectorize(math.erf)

        def ncdf(x):
            return Dual(0.5 * (1.0 + erf(x.v / math.sqrt(2.0))), np.exp(-0.5 * x.v * x.v) / math.sqrt(2.0 * math.pi) * x.d)

        for p in range(len(pr)):
            assert pr["n_states"][p] == 1
            for q in range(pr["ev_begin"][p], pr["ev_end"][p]):
                e = ev[q]
                if e["kind"] <= _abi.EV_EXERCISE:
                    continue
                v = None
                if e["kind"] == _abi.EV_EXPO_BS:
                    if e["aux"][2] > 0.0:
                        unit = lambda s_: np.array([1.0 if r == s_ else 0.0 for r in range(self.NP)])
                        sig = Dual.uniform(e["aux"][0], unit(ev_param[q][0] if ev_param is not None else -1), self.n, self.dtype)
                        rate = Dual.uniform(e["aux"][1], unit(ev_param[q][1] if ev_param is not None else -1), self.n, self.dtype)
                        tau, Kx, spot = float(e["aux"][2]), float(e["strike"]), self.atom(int(e["x_atom"]))
                        sq = math.sqrt(tau)
                        d1 = (dlog(spot / Kx) + (rate + sig * sig * 0.5) * tau) / (sig * sq)
                        d2 = d1 - sig * sq
                        df = dexp(rate * (-tau))
                        price = spot * ncdf(d1) - df * ncdf(d2) * Kx if e["sign"] > 0 else df * ncdf(d2 * -1.0) * Kx - spot * ncdf(d1 * -1.0)
                        v = price / self.atom(int(e["num_atom"]))
                elif e["coeff_off"] >= 0:
                    x, o = self.atom(int(e["x_atom"])), int(e["coeff_off"])
                    xp = Dual.uniform(self.dtype(1.0), np.zeros(self.NP), self.n, self.dtype)
                    for k in range(K):
                        t = Dual.uniform(self.dtype(coeffs[o + k]), dcoeffs[o + k], self.n, self.dtype) * xp
                        v = t if v is None else v + t
                        xp = xp * x
                    v = v / self.atom(int(e["num_atom"]))
                if v is not None:
                    out[0, pr["netting_set"][p], e["expo_row"]] += v.v
                    out[1:, pr["netting_set"][p], e["expo_row"]] += v.d
        return out

    def moments(self, product, first_event, num_atom, x_atom, shift, scale, K, terms=False, f32_cache=False):
        """[1 + NP][(2K-1) + K]: the dual normal equations of one (product, regression date) as mcx_tangent_lsm returns them — sums
        over the paths of z^k (k < 2K-1), then of z^k Y (k < K), Y = numeraire x the product's cash events from first_event on,
        z = (x - shift) scale.  terms: the per-path summands [1 + NP][NM][n] instead.  f32_cache: the VALUE of the cashflow sum is
        rounded to float32 after every product date, as the reference's cf_cache is (controller.py:312-330); tangents are not"""
        pr = self.plan.products
        total = None
        for q in range(pr["cf_begin"][product] + first_event, pr["cf_end"][product]):
            v = self.event(q)
            total = v if total is None else total + v
            if f32_cache:
                total = Dual(total.v.astype(np.float32).astype(self.dtype), total.d)
        if total is None:
            total = Dual.uniform(self.dtype(0.0), np.zeros(self.NP), self.n, self.dtype)
        y = self.atom(num_atom) * total
        z = (self.atom(x_atom) - self.dtype(shift)) * self.dtype(scale)
        zp = Dual.uniform(self.dtype(1.0), np.zeros(self.NP), self.n, self.dtype)
        out = np.zeros((1 + self.NP, (2 * K - 1) + K, self.n), dtype=self.dtype)
        for k in range(2 * K - 1):
            out[0, k], out[1:, k] = zp.v, zp.d
            if k < K:
                zy = zp * y
                out[0, 2 * K - 1 + k], out[1:, 2 * K - 1 + k] = zy.v, zy.d
            zp = zp * z
        return out if terms else out.sum(axis=-1)

    def smallest_margin(self):
        """the smallest distance of any path to a band edge (in band units), a payoff kink (absolute) or a tie among the monitored
        spots (relative), over the events evaluated so far; a path ON the flat side of a band has margin >= its distance too"""
        return min((float(np.min(a)) for arrs in self.margins.values() for a in arrs), default=np.inf)


def rounding_gap(make):
    """the yardstick's own rounding: the largest gap, relative to the row's largest entry, between the float64 and the longdouble
    run of the restatement.  make(dtype) -> cashflow image [1 + NP][n_ns][n]"""
    lo, hi = make(np.float64), make(np.longdouble)
    scale = np.max(np.abs(hi), axis=-1, keepdims=True)
    scale = np.where(scale == 0, 1.0, scale)
    return float(np.max(np.abs(lo.astype(np.longdouble) - hi) / scale))


def philox_bridge_uniforms(seed, path_offset, n, n_intervals, draw_id):
    """[2 * n_intervals][n]: the uniforms a bridge event draws itself — Philox4x32-10 with key = seed and counter (global path id,
    interval, 0x80000000 | (2 draw_id + barrier)), u = ((w1:w0 >> 11) + 0.5) 2^-53 (include/mcx.h "RNG contract")"""
    from step_cases import philox4x32_10
    path = np.uint64(path_offset) + np.arange(n, dtype=np.uint64)
    lo, hi = path & np.uint64(0xFFFFFFFF), path >> np.uint64(32)
    out = np.empty((2 * n_intervals, n))
    for k in range(n_intervals):
        for bi in range(2):
            w = philox4x32_10(lo, hi, np.uint64(k), np.uint64(0x80000000 | (2 * draw_id + bi)), seed & 0xFFFFFFFF, seed >> 32)
            out[2 * k + bi] = ((((w[1] << np.uint64(32)) | w[0]) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    return out
