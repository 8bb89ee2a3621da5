"""Plain numpy restatement of the FVA table (mcx/metrics/fva_metric.py, csrc/k4_fva.hip), in float64 or long double, and an
independent restatement of the funding-spread integral.

Inputs: x [E][n] unsecured exposures (signed, discounted), the two atom value arrays [E-1][n] (S_c(0,t_k), S_o(0,t_k); None for a
name that never defaults) and the two weight tables [E-1].  Per path, with the sums over k = 0 .. E-2:

    fca = sum relu(x_k) S_c S_o w_b(k)        fba = sum relu(-x_k) S_c S_o w_l(k)        fva = fca - fba
"""
import math

import numpy as np

from xva_reference import mean_and_error  # noqa: F401  (the records' reference, shared with the bilateral-xVA tests)

EVALUATIONS = ("fca", "fba", "fva")
# the two funding curves of the tests: tenors inside an interval of the 0.25-spaced metric timeline (0.3), on its dates and beyond
# its end (5.0; the lending curve ends before it, so its last value is extended)
BORROW_CURVE = {0.5: 0.012, 1.0: 0.015, 1.75: 0.02, 5.0: 0.025}
LEND_CURVE = {0.3: 0.004, 1.25: 0.006, 2.0: 0.009}


def integrands(x, S_c, S_o, w_b, w_l, dtype=np.float64):
    """[3][n] per-path integrands in `dtype`"""
    T = dtype
    x = np.asarray(x).astype(T)
    E, n = x.shape
    nd = max(E - 1, 0)
    Sc = np.ones((nd, n), dtype=T) if S_c is None else np.asarray(S_c).astype(T)
    So = np.ones((nd, n), dtype=T) if S_o is None else np.asarray(S_o).astype(T)
    wb, wl = (np.asarray(w, dtype=np.float64).astype(T).reshape(nd, 1) for w in (w_b, w_l))
    ep, en = np.maximum(x[:nd], 0), np.maximum(-x[:nd], 0)
    fca = (ep * (Sc * So) * wb).sum(axis=0)
    fba = (en * (Sc * So) * wl).sum(axis=0)
    return np.stack([fca, fba, fca - fba])


def spread_at(spread, u: float) -> float:
    """s(u): a flat value, or the curve's value on the segment t_{i-1} < u <= t_i (the last value beyond the last tenor)"""
    if not isinstance(spread, dict):
        return float(spread)
    for tenor, value in spread.items():
        if u <= tenor:
            return float(value)
    return float(list(spread.values())[-1])


def spread_integral(spread, t0: float, t1: float) -> float:
    """int_{t0}^{t1} s(u) du by cutting [t0, t1] at every tenor inside it and reading the curve at each piece's midpoint (the curve
    is constant on a piece, so this is exact); math.fsum over the pieces"""
    cuts = [float(t0)] + sorted(float(t) for t in (spread if isinstance(spread, dict) else ()) if t0 < t < t1) + [float(t1)]
    return math.fsum(spread_at(spread, 0.5 * (a + b)) * (b - a) for a, b in zip(cuts, cuts[1:]))


def funding_weights(spread, timeline):
    """[E-1] weights 1 - exp(-I_k), by long-double exp rounded to float64 (not expm1: another route to the same number)"""
    t = [float(v) for v in timeline]
    out = []
    for k in range(len(t) - 1):
        integral = np.longdouble(spread_integral(spread, t[k], t[k + 1]))
        out.append(float(np.longdouble(1.0) - np.exp(-integral)))
    return np.array(out, dtype=np.float64)
