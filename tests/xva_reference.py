"""Plain numpy restatement of the bilateral xVA table (mcx/metrics/bcva_metric.py, csrc/k4_xva.hip), in float64 or long double.

Inputs: x [E][n] unsecured exposures (signed, discounted), the four atom value arrays [E-1][n] (S_c, cs_c, S_o, cs_o with
S_n(k) = S_n(0, t_k), cs_n(k) = S_n(t_k, t_{k+1}); None for a name that never defaults) and the two recoveries.  Per path, with
q = 1 - cs and the sums over k = 0 .. E-2:

    cva = (1-R_c) sum relu(x_k) S_c q_c        dva = (1-R_o) sum relu(-x_k) S_o q_o
    cva_ftd = (1-R_c) sum relu(x_k) S_c q_c S_o        dva_ftd = (1-R_o) sum relu(-x_k) S_o q_o S_c        bcva = cva_ftd - dva_ftd
"""
import numpy as np

EVALUATIONS = ("cva", "dva", "cva_ftd", "dva_ftd", "bcva")


def integrands(x, S_c, cs_c, S_o, cs_o, R_c, R_o, dtype=np.float64):
    """[5][n] per-path integrands in `dtype`"""
    T = dtype
    x = np.asarray(x).astype(T)
    E, n = x.shape
    one = T(1.0)

    def side(S, cs):
        if S is None:
            return np.ones((max(E - 1, 0), n), dtype=T), np.zeros((max(E - 1, 0), n), dtype=T)
        return np.asarray(S).astype(T), one - np.asarray(cs).astype(T)

    (Sc, qc), (So, qo) = side(S_c, cs_c), side(S_o, cs_o)
    ep, en = np.maximum(x[:E - 1], 0), np.maximum(-x[:E - 1], 0)
    lc, lo = one - T(R_c), one - T(R_o)
    cva = lc * (ep * Sc * qc).sum(axis=0)
    dva = lo * (en * So * qo).sum(axis=0)
    cftd = lc * (ep * Sc * qc * So).sum(axis=0)
    dftd = lo * (en * So * qo * Sc).sum(axis=0)
    return np.stack([cva, dva, cftd, dftd, cftd - dftd])


def mean_and_error(v):
    """(mean, std(unbiased)/sqrt(n)) along the last axis, in the dtype of v (n == 1: error NaN, as torch gives)"""
    v = np.asarray(v)
    n = v.shape[-1]
    m = v.sum(axis=-1) / n
    if n < 2:
        return m, np.full_like(m, np.nan)
    d = v - m[..., None]
    return m, np.sqrt((d * d).sum(axis=-1) / (n - 1)) / np.sqrt(v.dtype.type(n))
