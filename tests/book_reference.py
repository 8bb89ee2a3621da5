"""A plain interpreter of the book program of include/mcx.h ("book program (K2)") in numpy long double.

TEST INFRASTRUCTURE.  It reads only the plan arrays (atoms, terms, events, products, coeffs) and a paths array and restates the
header, not a kernel: atoms a + d x + b exp(c0 + c1 x); event kinds 1-5; OPTION modes 0-3 (sum, geometric, control-variate
basket, fuzzy binary); per-term denominators; the exercise rule with exercise state and the FlexiCall rule; set-or-accumulate
per exposure row; netting-set sums; the want_cfs == 0 skip; record and replay of exercise bits.  Barrier events (modes 4, 5) are
not restated: `evaluate` raises on them (the CPU oracle is their reference).

Next to every cashflow and exposure entry it returns a magnitude M: the sum of the absolute values of everything added into the
entry, taken at the granularity at which the arithmetic rounds —
  atom          |a| + |d x| + |b| exp(c0 + c1 x)                                (a LIBOR atom cancels: (P1 / P2 - 1) / tau)
  term          |w| mag(atom) / |numeraire or den|
  option        (sum of its terms' magnitudes + |strike|) / |numeraire|, whether or not it pays (max(., 0) is 1-Lipschitz)
  geometric     (G (1 + sum |w log(atom + 1e-10)|) + |strike|) / |numeraire|,  G = exp(sum w log(atom + 1e-10))
  control var.  arithmetic + geometric + |aux1| / |numeraire|
  binary        |aux1| (sum of magnitudes + |strike| + aux2) / (2 aux2) / |numeraire|   (the ramp amplifies by 1 / (2 aux2))
  polynomial    sum_k |c_k x^k| / |numeraire|
  Black-Scholes (spot + K df) / |numeraire|
so that |computed - exact| <= tol * M is the statement "every operation rounded to a few ulps" also where a swap's legs cancel.
For exercise events it returns the decision margin imm + cont_ex - cont and its scale |imm| + |cont| + |cont_ex|; a path whose
margin lies within `band` times the scale is TIED from that event on: its netting set's cashflow and every exposure entry a later
event of that product writes are flagged in `*_tied` (a double-precision evaluation may decide the other way there)."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
# Tolerances of |computed - reference| <= TOL * M: four times the largest ratio measured on the books of tests/book_cases.py
# (DESIGN "The book kernels: what is pinned" lists the measurements).
TOL_ORACLE = 4 * 6.3e-16     # oracle/mcx_oracle.c (host libm, plain double): 6.26e-16 measured (tests/test_book_reference.py)
TOL_SCALAR = 4 * 6.2e-16     # k2_eval_book, k2_resolve (device libm): 6.19e-16 measured on the MI355X
TOL_MULTI = 4 * 5.6e-16      # k2_eval_book_v (table exponential, mcx_rcp): 5.57e-16 measured on the MI355X
TIE_BAND = 64.0              # an exercise margin within TIE_BAND * TOL of its scale is a tie
EV_CASHFLOW, EV_OPTION, EV_EXERCISE, EV_EXPO_POLY, EV_EXPO_BS = 1, 2, 3, 4, 5
_SQRT1_2 = LD(1) / np.sqrt(LD(2))
_TWO_OVER_SQRT_PI = LD(2) / np.sqrt(np.arccos(LD(-1)))


def erf_ld(x):
    """erf in long double: 2/sqrt(pi) exp(-x^2) sum_n 2^n x^(2n+1) / (1 3 5 .. (2n+1)) — every term of one sign, no cancellation;
    |x| >= 6.6: +-1 to 1e-19"""
    x = np.asarray(x, dtype=LD)
    ax = np.minimum(np.abs(x), LD(6.6))
    term = ax.copy()
    total = ax.copy()
    x2 = 2 * ax * ax
    for n in range(1, 400):
        term = term * x2 / (2 * n + 1)
        total = total + term
        if not (term > total * LD(1e-22)).any():
            break
    r = np.minimum(_TWO_OVER_SQRT_PI * np.exp(-ax * ax) * total, LD(1))
    return np.where(x < 0, -r, r)


def norm_cdf_ld(x):
    return LD(0.5) * (1 + erf_ld(np.asarray(x, dtype=LD) * _SQRT1_2))


class Result:
    """cfs / expo: values [NS][m] / [NS][E][m] (long double); *_M: magnitudes; *_tied: bool, entry not comparable (exercise tie);
    written [NS][E]: some event writes the row; decisions / margins / scales / live / tie_at: per exercise event index q, [m]
    arrays (live: the path still had a right, s > 0, so the decision was taken; tie_at: the margin is inside the band); final_state [n_products][m]; atoms: {id: (value, mag)}"""


def atom(plan, k, P):
    """(value, magnitude) of atom k on the gathered paths P [T][D][m] (float64)"""
    a = plan.atoms[k]
    m = P.shape[2]
    x = P[int(a["t_idx"]), int(a["col"])].astype(LD) if a["col"] >= 0 else np.zeros(m, dtype=LD)
    lin = LD(a["d"]) * x
    e = LD(a["b"]) * np.exp(LD(a["c0"]) + LD(a["c1"]) * x) if a["b"] != 0.0 else np.zeros(m, dtype=LD)
    return LD(a["a"]) + lin + e, abs(LD(a["a"])) + np.abs(lin) + np.abs(e)


def _poly(coeffs, off, s, K, x):
    """(sum_k c[off + s K + k] x^k, sum_k |c x^k|) with a per-path state s"""
    v = np.zeros(len(x), dtype=LD)
    mag = np.zeros(len(x), dtype=LD)
    xp = np.ones(len(x), dtype=LD)
    for k in range(K):
        t = coeffs[off + s * K + k].astype(LD) * xp
        v += t
        mag += np.abs(t)
        xp = xp * x
    return v, mag


def evaluate(plan, P, band=0.0, replay=None, coeffs=None):
    """the book `plan` on the gathered paths P [T][D][m].  replay: {event index: bool [m]} exercise bits to follow instead of the
    rule (as mcx_book_set_exercise_replay mode 2; no ties then).  coeffs: override of plan.coeffs."""
    coeffs = np.asarray(plan.coeffs if coeffs is None else coeffs, dtype=np.float64)
    K, NS, E = plan.n_basis, plan.n_netting_sets, plan.n_expo_rows
    want_cfs, want_expo = bool(plan.desc.want_cfs), bool(plan.desc.want_expo)
    m = P.shape[2]
    cache = {}

    def at(k):
        if k not in cache:
            cache[k] = atom(plan, int(k), P)
        return cache[k]

    res = Result()
    res.cfs, res.cfs_M = np.zeros((NS, m), dtype=LD), np.zeros((NS, m), dtype=LD)
    res.cfs_tied = np.zeros((NS, m), dtype=bool)
    res.expo, res.expo_M = np.zeros((NS, E, m), dtype=LD), np.zeros((NS, E, m), dtype=LD)
    res.expo_tied = np.zeros((NS, E, m), dtype=bool)
    res.written = np.zeros((NS, E), dtype=bool)
    res.decisions, res.margins, res.scales, res.live, res.tie_at = {}, {}, {}, {}, {}
    res.final_state = np.zeros((len(plan.products), m), dtype=np.int64)
    zero = np.zeros(m, dtype=LD)
    for p_i, pr in enumerate(plan.products):
        ns = int(pr["netting_set"])
        s = np.full(m, int(pr["init_state"]), dtype=np.int64)
        tied = np.zeros(m, dtype=bool)
        for q in range(int(pr["ev_begin"]), int(pr["ev_end"])):
            e = plan.events[q]
            kind, aux = int(e["kind"]), e["aux"]
            if kind <= EV_EXERCISE:
                if not want_cfs and int(pr["n_states"]) == 1 and kind != EV_EXERCISE:
                    continue                 # feeds the cashflow output alone
                if kind == EV_OPTION and aux[0] in (4.0, 5.0):
                    raise NotImplementedError("barrier events are not restated: the oracle is their reference")
                num, num_mag = at(e["num_atom"])
                ncond = num_mag / np.abs(num)               # 1 for a pure exponential
                common, common_mag, own, own_mag = zero.copy(), zero.copy(), zero.copy(), zero.copy()
                glog, glog_mag = zero.copy(), zero.copy()
                for j in range(int(e["term_begin"]), int(e["term_end"])):
                    tm = plan.terms[j]
                    av, amag = at(tm["atom"])
                    w = LD(tm["w"])
                    if tm["den"] >= 0:
                        assert kind == EV_CASHFLOW
                        dn, dmag = at(tm["den"])
                        own += w * av / dn
                        own_mag += abs(w) * amag / np.abs(dn) * (dmag / np.abs(dn))
                    else:
                        common += w * av
                        common_mag += abs(w) * amag
                    if kind == EV_OPTION and aux[0] in (1.0, 2.0):
                        lg = np.log(av + LD(1e-10))
                        glog += w * lg
                        glog_mag += abs(w) * (np.abs(lg) + amag / np.abs(av + LD(1e-10)))
                if kind == EV_CASHFLOW:
                    v, M = common / num + own, common_mag / np.abs(num) * ncond + own_mag
                else:
                    strike, sign = LD(e["strike"]), LD(e["sign"])
                    imm = np.maximum(sign * (common - strike), 0)
                    imm_M = (common_mag + abs(strike)) / np.abs(num) * ncond
                    if kind == EV_OPTION and aux[0] == 3.0:
                        dot = np.clip((common - strike + LD(aux[2])) / (2 * LD(aux[2])), 0, 1)
                        v = LD(aux[1]) * (dot if sign > 0 else 1 - dot) / num
                        M = abs(LD(aux[1])) * (common_mag + abs(strike) + abs(LD(aux[2]))) / (2 * LD(aux[2])) / np.abs(num) * ncond
                    elif kind == EV_OPTION and aux[0] != 0.0:
                        G = np.exp(glog)
                        geo = np.maximum(sign * (G - strike), 0)
                        geo_M = (G * (1 + glog_mag) + abs(strike)) / np.abs(num) * ncond
                        if aux[0] == 1.0:
                            v, M = geo / num, geo_M
                        else:
                            v, M = (imm - geo + LD(aux[1])) / num, imm_M + geo_M + abs(LD(aux[1])) / np.abs(num)
                    elif kind == EV_OPTION:
                        v, M = imm / num, imm_M
                    else:                                   # EV_EXERCISE
                        cont, cont_ex = zero.copy(), zero.copy()
                        if e["coeff_off"] >= 0:
                            x, _ = at(e["x_atom"])
                            cont, _ = _poly(coeffs, int(e["coeff_off"]), s, K, x)
                            if aux[0] == 1.0:
                                ce, _ = _poly(coeffs, int(e["coeff_off"]), np.maximum(s - 1, 0), K, x)
                                cont_ex = np.where(s > 0, ce, 0)
                        margin = imm + cont_ex - cont
                        scale = np.abs(imm) + np.abs(cont) + np.abs(cont_ex)
                        live = s > 0
                        if replay is not None:
                            ex = np.asarray(replay[q], dtype=bool) & live
                        else:
                            ex = (margin > 0) & live
                            # (scale == 0: nothing to weigh — out of the money on a date without continuation values; every
                            #  precision decides "no" unless the payoff's own argument is within rounding of zero)
                            raw_tie = np.abs(sign * (common - strike)) <= LD(band) * (common_mag + abs(strike))
                            res.tie_at[q] = live & (np.abs(margin) <= LD(band) * scale) & ((scale > 0) | raw_tie)
                            tied |= res.tie_at[q]
                        res.decisions[q], res.margins[q], res.scales[q], res.live[q] = ex, margin, scale, live
                        s = s - ex
                        v, M = np.where(ex, imm / num, 0), imm_M
                res.cfs[ns] += v
                res.cfs_M[ns] += M
            else:
                row = int(e["expo_row"])
                v, M = zero, zero
                if kind == EV_EXPO_POLY:
                    if e["coeff_off"] >= 0:
                        num, num_mag = at(e["num_atom"])
                        x, _ = at(e["x_atom"])
                        pv, pm = _poly(coeffs, int(e["coeff_off"]), s, K, x)
                        v, M = pv / num, pm / np.abs(num) * (num_mag / np.abs(num))
                elif aux[2] > 0.0:                          # EV_EXPO_BS
                    num, num_mag = at(e["num_atom"])
                    spot, _ = at(e["x_atom"])
                    sig, rate, tau, Kx = LD(aux[0]), LD(aux[1]), LD(aux[2]), LD(e["strike"])
                    sq = np.sqrt(tau)
                    d1 = (np.log(spot / Kx) + (rate + LD(0.5) * sig * sig) * tau) / (sig * sq)
                    d2 = d1 - sig * sq
                    df = np.exp(-rate * tau)
                    if e["sign"] > 0.0:
                        price = spot * norm_cdf_ld(d1) - Kx * df * norm_cdf_ld(d2)
                    else:
                        price = Kx * df * norm_cdf_ld(-d2) - spot * norm_cdf_ld(-d1)
                    v, M = price / num, (np.abs(spot) + abs(Kx) * df) / np.abs(num) * (num_mag / np.abs(num))
                res.expo[ns, row] += v
                res.expo_M[ns, row] += M
                res.expo_tied[ns, row] |= tied
                res.written[ns, row] = True
        res.cfs_tied[ns] |= tied
        res.final_state[p_i] = s
    res.atoms = cache
    return res


def nan_unused_rows(paths, used):
    """NaN in every (date, state) row of the paths tensor no atom names (a kernel that reads one shows it)"""
    for t in range(paths.shape[0]):
        for c in range(paths.shape[1]):
            if (t, c) not in used:
                paths[t, c] = float("nan")


def worst_ratio(got, ref, M, skip=None):
    """max |got - ref| / M over the entries not skipped (M == 0: the entry must be exact)"""
    err = np.abs(got.astype(LD) - ref)
    ok = np.ones(err.shape, dtype=bool) if skip is None else ~skip
    assert not (err[ok & (M == 0)] != 0).any()
    pos = ok & (M > 0)
    return float((err[pos] / M[pos]).max()) if pos.any() else 0.0
