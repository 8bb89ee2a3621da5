"""A plain interpreter of the DUAL book program in numpy: what the kernels of csrc/kt_book.hip downstream of the paths should compute.

TEST INFRASTRUCTURE.  It reads the plan arrays (atoms, terms, events, products), a paths array with its tangents and the tangents
of the atoms and of the regression coefficients, and restates include/mcx.h ("book program") and the reference's tape conventions,
not a kernel.  Every number is a pair (value [n], tangents [NP][n]) in `dtype` (np.float64 or np.longdouble):

  atom        a + d x + b exp(c0 + c1 x): the five numbers take their tangents from datoms[atom][5][NP], x from dpaths
  term sum    a term with den >= 0 is divided by its OWN dual denominator atom and kept apart from the numeraire division
  CASHFLOW    common / numeraire + own
  OPTION      mode 0: max((val - strike) sign, 0) / numeraire; gradient 1 above the kink, 0 below, 1/2 at the tie (torch.maximum)
  EXERCISE    the decision is taken from VALUES (immediate value, continuation polynomial of the path's state with the primal
              coefficients; FlexiCall: plus the continuation of state s - 1) and only while s > 0; the tangent flows through the
              taken branch only; the state is decremented
  EXPO_POLY   sum_k c_k x^k / numeraire with dual coefficients (coeffs, dcoeffs[n][NP]); the row of the path's current exercise
              state where the product has states, row 0 otherwise
  EXPO_BS     the Black-Scholes price of the remaining option over the numeraire; sigma and rate are seeded with 1 in the slots
              ev_param[q] names (-1: none); no contribution when aux[2] == 0

and, for the metric kernels, `unsecured` / `cva` / `profiles` / `pick` on an exposure array [1+NP][rows][n] of one netting set
(netting_set.py: strict > h and < -h, zero value and zero tangent on the closed band, nothing thresholded at h == 0, a
collateralised date without a delayed row is the exposure itself).

Margins.  Next to the values the interpreter records how far every path is from each decision edge, relative to the scale of the
compared quantity: `kinks[q]` = |sign (val - strike)| / (sum |term| + |strike|) of an option or exercise payoff, `margins[q, s]` =
|imm + cont_ex - cont| / (|imm| + |cont| + |cont_ex|) of an exercise decision in state s (inf where nothing is weighed), and
the `margins` list of `unsecured` / `cva` takes |u| and ||e| - h| of the metric functions.  A float64 evaluation may decide the other way only inside them."""
import math

import numpy as np

import book_reference as R
from payoff_tangent_reference import Dual, dexp, dlog, dmax0

LD = np.longdouble
EV_CASHFLOW, EV_OPTION, EV_EXERCISE, EV_EXPO_POLY, EV_EXPO_BS = 1, 2, 3, 4, 5
_erf64 = np.vectorize(math.erf, otypes=[np.float64])


class Run:
    """cfs [1+NP][NS][n], expo [1+NP][NS][rows][n]; cfs_mag / expo_mag: the sum of the |event| added into every entry, image by image
    (an entry far below it cancels between events: its rounding error is that of the magnitude); decisions {event: bool [n]};
    final_state [n_products][n]; row_state {exposure event: state [n] whose coefficient row it took}"""


def _norm_cdf(x, dtype):
    return R.norm_cdf_ld(x) if dtype is LD else 0.5 * (1.0 + _erf64(x / math.sqrt(2.0)))


class DualBook:
    def __init__(self, plan, paths, dpaths, datoms, dtype=LD):
        self.plan, self.dtype = plan, dtype
        self.paths, self.dpaths = np.asarray(paths, dtype=dtype), np.asarray(dpaths, dtype=dtype)
        self.datoms = np.asarray(datoms, dtype=dtype)
        self.NP, self.n = self.dpaths.shape[0], self.paths.shape[2]
        assert self.dpaths.shape[1:] == self.paths.shape and self.datoms.shape == (len(plan.atoms), 5, self.NP)
        self._atoms = {}
        self.kinks, self.margins = {}, {}

    # ---- atoms and terms ------------------------------------------------------------------------------------------------------
    def uniform(self, c, dc=None):
        return Dual.uniform(self.dtype(c), np.zeros(self.NP) if dc is None else dc, self.n, self.dtype)

    def atom_mag(self, k):
        """(dual value, magnitude |a| + |d x| + |b exp(.)|) of atom k"""
        k = int(k)
        if k not in self._atoms:
            a, da = self.plan.atoms[k], self.datoms[k]
            if a["col"] >= 0:
                x = Dual(self.paths[int(a["t_idx"]), int(a["col"])].copy(), self.dpaths[:, int(a["t_idx"]), int(a["col"])].copy())
            else:
                x = self.uniform(0.0)
            lin = self.uniform(a["d"], da[1]) * x
            v = self.uniform(a["a"], da[0]) + lin
            mag = abs(self.dtype(a["a"])) + np.abs(lin.v)
            if a["b"] != 0.0:
                e = self.uniform(a["b"], da[2]) * dexp(self.uniform(a["c0"], da[3]) + self.uniform(a["c1"], da[4]) * x)
                v, mag = v + e, mag + np.abs(e.v)
            self._atoms[k] = (v, mag)
        return self._atoms[k]

    def atom(self, k):
        return self.atom_mag(k)[0]

    def term_sum(self, e):
        """(sum over the numeraire, sum of the terms over their own denominators, sum |w| mag(atom) of the former)"""
        val, own, mag = self.uniform(0.0), self.uniform(0.0), np.zeros(self.n, dtype=self.dtype)
        for j in range(int(e["term_begin"]), int(e["term_end"])):
            tm = self.plan.terms[j]
            av, am = self.atom_mag(tm["atom"])
            v = av * self.dtype(tm["w"])
            if tm["den"] < 0:
                val, mag = val + v, mag + abs(self.dtype(tm["w"])) * am
            else:
                own = own + v / self.atom(tm["den"])
        return val, own, mag

    def n_terms(self, q):
        """terms of event q as the floor of the yardstick counts them: the weighted atoms of a cash or exercise event, the n_basis
        monomials of a polynomial exposure, the two legs spot N(d1) and K df N(d2) of a Black-Scholes exposure"""
        e = self.plan.events[q]
        if e["kind"] == EV_EXPO_POLY:
            return int(self.plan.n_basis)
        if e["kind"] == EV_EXPO_BS:
            return 2
        return int(e["term_end"]) - int(e["term_begin"])

    def longest(self, q0, q1):
        """terms of the longest event in [q0, q1)"""
        return max([self.n_terms(q) for q in range(int(q0), int(q1))] + [0])

    # ---- events ---------------------------------------------------------------------------------------------------------------
    def _payoff(self, q, e, val, mag):
        arg = (val - self.dtype(e["strike"])) * self.dtype(e["sign"])
        self.kinks[q] = np.abs(arg.v) / (mag + abs(self.dtype(e["strike"])))
        return dmax0(arg)

    def cash_event(self, q):
        """normalised dual cashflow of a CASHFLOW event or an OPTION event in mode 0"""
        e = self.plan.events[q]
        num = self.atom(e["num_atom"])
        val, own, mag = self.term_sum(e)
        if e["kind"] == EV_CASHFLOW:
            return val / num + own
        if e["kind"] != EV_OPTION or e["aux"][0] != 0.0:
            raise NotImplementedError("OPTION modes 1-5 are restated in payoff_tangent_reference.py")
        assert all(self.plan.terms["den"][j] < 0 for j in range(int(e["term_begin"]), int(e["term_end"])))
        return self._payoff(q, e, val, mag) / num

    def exercise_value(self, q):
        """(dual immediate value over the numeraire, immediate VALUE, VALUE of the explanatory variable)"""
        e = self.plan.events[q]
        val, _own, mag = self.term_sum(e)
        assert all(self.plan.terms["den"][j] < 0 for j in range(int(e["term_begin"]), int(e["term_end"])))
        imm = self._payoff(q, e, val, mag)
        x = self.atom(e["x_atom"]).v if e["coeff_off"] >= 0 else np.zeros(self.n, dtype=self.dtype)
        return imm / self.atom(e["num_atom"]), imm.v, x

    def _poly(self, coeffs, off, s, x):
        K = self.plan.n_basis
        v, xp = np.zeros(self.n, dtype=self.dtype), np.ones(self.n, dtype=self.dtype)
        for k in range(K):
            v = v + np.asarray(coeffs, dtype=self.dtype)[off + s * K + k] * xp
            xp = xp * x
        return v

    def decide(self, q, imm, x, s, coeffs):
        """exercise decision of the paths in state s [n] (values only; PRIMAL coefficients)"""
        e = self.plan.events[q]
        zero = np.zeros(self.n, dtype=self.dtype)
        cont, cont_ex = zero, zero
        if e["coeff_off"] >= 0:
            cont = self._poly(coeffs, int(e["coeff_off"]), s, x)
            if e["aux"][0] == 1.0:                                                    # FlexiCall: the continuation one right less
                cont_ex = np.where(s > 0, self._poly(coeffs, int(e["coeff_off"]), np.maximum(s - 1, 0), x), zero)
        margin, scale = imm + cont_ex - cont, np.abs(imm) + np.abs(cont) + np.abs(cont_ex)
        live = s > 0
        rel = np.full(self.n, np.inf)
        ok = live & (scale > 0)
        rel[ok] = (np.abs(margin[ok]) / scale[ok]).astype(np.float64)
        for st in np.unique(s):
            prev = self.margins.get((q, int(st)))
            cur = np.where(s == st, rel, np.inf)
            self.margins[q, int(st)] = cur if prev is None else np.minimum(prev, cur)
        return (margin > 0) & live

    def evaluate(self, coeffs, dcoeffs, ev_param=None):
        plan, dt = self.plan, self.dtype
        K, NS, rows = plan.n_basis, plan.n_netting_sets, max(int(plan.n_expo_rows), 1)
        coeffs, dcoeffs = np.asarray(coeffs, dtype=dt), np.asarray(dcoeffs, dtype=dt)
        out = Run()
        out.cfs = np.zeros((1 + self.NP, NS, self.n), dtype=dt)
        out.expo = np.zeros((1 + self.NP, NS, rows, self.n), dtype=dt)
        out.cfs_mag, out.expo_mag = np.zeros_like(out.cfs), np.zeros_like(out.expo)
        out.cfs_terms, out.expo_terms = np.zeros(NS, dtype=np.int64), np.zeros((NS, rows), dtype=np.int64)     # longest event of the row

        def add(total, mag, v):
            total[0] += v.v
            total[1:] += v.d
            mag[0] += np.abs(v.v)
            mag[1:] += np.abs(v.d)
        out.decisions, out.row_state = {}, {}
        out.final_state = np.zeros((len(plan.products), self.n), dtype=np.int64)
        for p_i, pr in enumerate(plan.products):
            ns = int(pr["netting_set"])
            s = np.full(self.n, int(pr["init_state"]), dtype=np.int64)
            for q in range(int(pr["ev_begin"]), int(pr["ev_end"])):
                e = plan.events[q]
                kind = int(e["kind"])
                if kind <= EV_EXERCISE:
                    out.cfs_terms[ns] = max(out.cfs_terms[ns], self.n_terms(q))
                else:
                    out.expo_terms[ns, int(e["expo_row"])] = max(out.expo_terms[ns, int(e["expo_row"])], self.n_terms(q))
                if kind <= EV_OPTION:
                    add(out.cfs[:, ns], out.cfs_mag[:, ns], self.cash_event(q))
                elif kind == EV_EXERCISE:
                    pay, imm, x = self.exercise_value(q)
                    ex = self.decide(q, imm, x, s, coeffs)
                    out.decisions[q] = ex
                    add(out.cfs[:, ns], out.cfs_mag[:, ns], Dual(np.where(ex, pay.v, 0), np.where(ex, pay.d, 0)))
                    s = s - ex
                else:
                    v = self.uniform(0.0)
                    if kind == EV_EXPO_BS:
                        if e["aux"][2] > 0.0:
                            v = self._bs(q, e, ev_param)
                    elif e["coeff_off"] >= 0:
                        x = self.atom(e["x_atom"])
                        st = s if pr["n_states"] > 1 else np.zeros(self.n, dtype=np.int64)
                        out.row_state[q] = st.copy()
                        xp = self.uniform(1.0)
                        for k in range(K):
                            idx = int(e["coeff_off"]) + st * K + k
                            v = v + Dual(coeffs[idx], dcoeffs[idx].T.copy()) * xp
                            xp = xp * x
                        v = v / self.atom(e["num_atom"])
                    add(out.expo[:, ns, int(e["expo_row"])], out.expo_mag[:, ns, int(e["expo_row"])], v)
            out.final_state[p_i] = s
        return out

    def _bs(self, q, e, ev_param):
        dt = self.dtype
        unit = lambda slot: np.array([1.0 if r == slot else 0.0 for r in range(self.NP)])
        s_sig, s_rate = (int(ev_param[q][0]), int(ev_param[q][1])) if ev_param is not None else (-1, -1)
        sig, rate = self.uniform(e["aux"][0], unit(s_sig)), self.uniform(e["aux"][1], unit(s_rate))
        tau, Kx = dt(e["aux"][2]), dt(e["strike"])
        sq = np.sqrt(tau)
        spot = self.atom(e["x_atom"])
        d1 = (dlog(spot / Kx) + (rate + sig * sig * dt(0.5)) * tau) / (sig * sq)
        d2 = d1 - sig * sq
        df = dexp(rate * (-tau))

        def ncdf(x):
            pdf = np.exp(-x.v * x.v / 2) / np.sqrt(2 * np.arccos(dt(-1)))
            return Dual(_norm_cdf(x.v, dt).astype(dt), pdf * x.d)

        if e["sign"] > 0.0:
            price = spot * ncdf(d1) - df * ncdf(d2) * Kx
        else:
            price = df * ncdf(d2 * -1.0) * Kx - spot * ncdf(d1 * -1.0)
        return price / self.atom(e["num_atom"])

    # ---- one step of the regression of an exercise product (controller.py:316-383) -------------------------------------------------
    def lsm_step(self, product, roll_begin, roll_end, num_atom, x_atom, shift, scale, W, dW, coeffs, terms=False):
        """W [S][n], dW [NP][S][n]: discounted cashflows after the previous regression date per hypothetical state.  The window
        [roll_begin, roll_end) of the product's regression events is rolled along the frozen policy from EVERY hypothetical start
        state; the cached tail is looked up by the state the roll ends in.  -> (W', dW', moments [1+NP][(2K-1) + S K]; with
        terms=True the per-path summands [1+NP][NM][n] instead of their sums)"""
        plan, dt = self.plan, self.dtype
        pr = plan.products[product]
        K, S = plan.n_basis, int(pr["n_states"])
        W, dW = np.asarray(W, dtype=dt), np.asarray(dW, dtype=dt)
        assert W.shape == (S, self.n) and dW.shape == (self.NP, S, self.n)
        Wn, dWn = W.copy(), dW.copy()
        if roll_end > roll_begin:
            st = [np.full(self.n, s0, dtype=np.int64) for s0 in range(S)]
            sv = [self.uniform(0.0) for _ in range(S)]
            for q in range(int(pr["cf_begin"]) + roll_begin, int(pr["cf_begin"]) + roll_end):
                if plan.events["kind"][q] == EV_EXERCISE:
                    pay, imm, x = self.exercise_value(q)
                    for s0 in range(S):
                        ex = self.decide(q, imm, x, st[s0], coeffs)
                        sv[s0] = sv[s0] + Dual(np.where(ex, pay.v, 0), np.where(ex, pay.d, 0))
                        st[s0] = st[s0] - ex
                else:
                    v = self.cash_event(q)
                    sv = [a + v for a in sv]
            cols = np.arange(self.n)
            for s0 in range(S):
                Wn[s0] = sv[s0].v + W[st[s0], cols]
                dWn[:, s0] = sv[s0].d + dW[:, st[s0], cols]
        num = self.atom(num_atom)
        z = (self.atom(x_atom) - dt(shift)) * dt(scale)
        NM = (2 * K - 1) + S * K
        t = np.zeros((1 + self.NP, NM, self.n), dtype=dt)
        zp = self.uniform(1.0)
        for k in range(2 * K - 1):
            t[0, k], t[1:, k] = zp.v, zp.d
            if k < K:
                for s in range(S):
                    zy = zp * (num * Dual(Wn[s], dWn[:, s]))
                    t[0, 2 * K - 1 + s * K + k], t[1:, 2 * K - 1 + s * K + k] = zy.v, zy.d
            zp = zp * z
        return Wn, dWn, (t if terms else t.sum(axis=-1))

    def smallest_margin(self):
        """the smallest relative distance of any path to a payoff kink or an exercise tie over everything evaluated so far"""
        return min([float(np.min(a)) for a in self.kinks.values()] + [float(np.min(a)) for a in self.margins.values()], default=np.inf)


# ---- the metric functions on the exposures of one netting set, expo [1+NP][rows][n] ----------------------------------------------
def thr(e, h):
    if h == 0.0:
        return e
    up, dn = e.v > h, e.v < -h
    zero = np.zeros_like(e.v)
    return Dual(np.where(up, e.v - h, np.where(dn, e.v + h, zero)), np.where(up | dn, e.d, np.zeros_like(e.d)))


def unsecured(expo, row, threshold, collateralized=False, delayed=-1, dtype=LD, margins=None):
    """unsecured exposure of one metric date: thr(E[row]) when not collateralised, E[row] - thr(E[delayed]) when collateralised
    (delayed < 0: no collateral yet, the exposure itself).  margins: a list that takes ||e| - h| of the thresholded row"""
    expo = np.asarray(expo, dtype=dtype)
    h = dtype(threshold)
    e = Dual(expo[0, row], expo[1:, row])
    if not collateralized:
        if margins is not None and threshold != 0.0:
            margins.append(np.abs(np.abs(e.v) - h))
        return thr(e, h)
    if delayed is None or delayed < 0:
        return e
    dl = Dual(expo[0, delayed], expo[1:, delayed])
    if margins is not None and threshold != 0.0:
        margins.append(np.abs(np.abs(dl.v) - h))
    return e - thr(dl, h)


def _delayed(delayed, m):
    return -1 if delayed is None else int(delayed[m])


def cva(book, expo, rows, surv, cond, threshold, recovery, collateralized=False, delayed=None, margins=None, with_mag=False):
    """[1+NP][n] per path: sum over the dates m < n_dates - 1 with unsecured exposure > 0 of pos surv_m (1 - cond_m), times
    1 - recovery (cva_metric.py:62-100).  book: the DualBook whose atoms surv / cond name.  with_mag: also the sum of the |summand|
    of every entry, image by image"""
    dt = book.dtype
    total = book.uniform(0.0)
    mag = np.zeros((1 + book.NP, book.n), dtype=dt)
    for m in range(len(rows) - 1):
        u = unsecured(expo, int(rows[m]), threshold, collateralized, _delayed(delayed, m), dt, margins)
        if margins is not None:
            margins.append(np.abs(u.v))
        pos = u.v > 0
        t = u * book.atom(int(surv[m])) * (1.0 - book.atom(int(cond[m])))
        total = total + Dual(np.where(pos, t.v, 0), np.where(pos, t.d, 0))
        mag += np.where(pos, np.abs(np.concatenate([t.v[None], t.d])), 0)
    total = total * (dt(1.0) - dt(recovery))
    out = np.concatenate([total.v[None], total.d])
    return (out, mag * abs(dt(1.0) - dt(recovery))) if with_mag else out


def profiles(expo, rows, threshold, collateralized=False, delayed=None, dtype=LD, terms=False):
    """[n_dates][2][NP]: sums over the paths of 1[u > 0] du and 1[u < 0] du (terms=True: the summands [n_dates][2][NP][n])"""
    out = []
    for m in range(len(rows)):
        u = unsecured(expo, int(rows[m]), threshold, collateralized, _delayed(delayed, m), dtype)
        out.append(np.stack([np.where(u.v > 0, u.d, 0), np.where(u.v < 0, u.d, 0)]))
    out = np.stack(out)
    return out if terms else out.sum(axis=-1)


def pick(expo, rows, threshold, targets, collateralized=False, delayed=None, dtype=np.float64):
    """[n_dates][1+NP]: the smallest path index with u == target and its tangent, or (-1, 0 ..)"""
    NP = np.asarray(expo).shape[0] - 1
    out = np.zeros((len(rows), 1 + NP))
    for m in range(len(rows)):
        u = unsecured(expo, int(rows[m]), threshold, collateralized, _delayed(delayed, m), dtype)
        hit = np.nonzero(u.v == dtype(targets[m]))[0]
        out[m, 0] = -1.0
        if hit.size:
            out[m, 0] = float(hit[0])
            out[m, 1:] = u.d[:, hit[0]]
    return out


# ---- the per-path bound ------------------------------------------------------------------------------------------------------------
def row_gap(got, want):
    """largest |got - want| relative to the largest |want| of its row (the last axis: the compared paths)"""
    want = np.asarray(want, dtype=LD)
    scale = np.max(np.abs(want), axis=-1, keepdims=True)
    gap = np.abs(np.asarray(got).astype(LD) - want) / np.where(scale == 0, LD(1), scale)
    return float(np.max(gap)) if gap.size else 0.0


def row_condition(want, mag):
    """per row: the largest magnitude of the row over its largest |entry| (>= 1; 1 for a row nobody writes)"""
    top = np.max(np.abs(np.asarray(want, dtype=LD)), axis=-1)
    return np.asarray(np.where(top > 0, np.max(np.asarray(mag, dtype=LD), axis=-1) / np.where(top > 0, top, 1), 1), dtype=np.float64)


def row_gaps(got, want):
    """row_gap per row (all axes but the last)"""
    want = np.asarray(want, dtype=LD)
    scale = np.max(np.abs(want), axis=-1)
    return np.asarray(np.max(np.abs(np.asarray(got).astype(LD) - want), axis=-1) / np.where(scale == 0, LD(1), scale), dtype=np.float64)


def floor(n_terms):
    """the rounding of one event of n_terms terms: 2^-52 (n_terms + 4)"""
    return 2.0 ** -52 * (np.asarray(n_terms, dtype=np.float64) + 4)


def yardstick(lo, hi, n_terms):
    """the restatement's own rounding: row_gap of its float64 run against its long-double run, floored at 2^-52 (n_terms + 4),
    n_terms the terms of the longest event that writes the compared rows (DualBook.n_terms; for the CVA the three factors of a
    date's summand), so that rows whose float64 run happens to be exact do not bound a fused multiply-add"""
    return max(row_gap(lo, hi), float(np.max(floor(n_terms))))


FACTOR = 4.0                  # bound = 4 yardsticks: the device's exp / log / erf differ from numpy's by ulps
TIE_FACTOR = 64.0             # no path within 64 bounds of a kink or an exercise tie (a condition on the inputs)


def row_bounds(want, mag, y, n_terms):
    """the bound of every row: 4 yardsticks, or, where the row's entries cancel (between the events of a book row, between the dates
    of a CVA), the condition number of the row times the rounding of one event, 2^-52 (n_terms + 4), n_terms per row or for all
    (every event is a sum of its terms, products of correctly rounded operations and of exponentials good to an ulp, divided once;
    their errors add up over the magnitude, not over the entry)"""
    return np.maximum(FACTOR * y, row_condition(want, mag) * floor(n_terms))
