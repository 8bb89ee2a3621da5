"""Plain high-precision references for the Longstaff-Schwartz regression (test helpers, no kernel arithmetic shared).

* `exact_sum`: the sum of a float64 / longdouble vector to ~1e-19 relative to the sum of |terms| (each term split into two
  doubles, the halves summed by math.fsum, which rounds the exact sum once);
* `moments_ref`: the moment vector [sum z^k (k < 2K-1) | sum z^k Y_s (k < K) per state] that the moment kernels form, with the
  sum of |term| of every entry (the scale of its rounding error);
* `solve_ref`: the normal equations and the back-transformation z^k = scale^k (x - shift)^k in mpmath at 50 digits, with cond(G);
* `synthetic_moments`: moments of sampled z for the solver tests (well-conditioned, clustered, shifted / scaled)."""
import math

import mpmath
import numpy as np

EPS = float(np.finfo(np.float64).eps)
MP_DPS = 50


def exact_sum(t) -> float:
    t = np.asarray(t)
    if t.size == 0:
        return 0.0
    hi = t.astype(np.float64)
    lo = (t - hi.astype(t.dtype)).astype(np.float64)
    return math.fsum(np.concatenate([hi, lo]).tolist())


def moments_ref(z: np.ndarray, Y: np.ndarray, K: int):
    """z [n] (float64, as the kernel forms it), Y [S][n] (float64) -> (moments [(2K-1) + S K], sum |term| per moment).  Powers in
    long double (64-bit mantissa on x86-64): their error, ~k 2^-64 relative, is far below the kernels' float64 rounding."""
    z = np.asarray(z, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, z.size)
    zl = z.astype(np.longdouble)
    pw = [np.ones_like(zl)]
    for _ in range(2 * K - 2):
        pw.append(pw[-1] * zl)
    ref, mag = [], []
    for k in range(2 * K - 1):
        ref.append(exact_sum(pw[k]))
        mag.append(float(np.abs(pw[k]).sum()))
    for s in range(Y.shape[0]):
        yl = Y[s].astype(np.longdouble)
        for k in range(K):
            t = pw[k] * yl
            ref.append(exact_sum(t))
            mag.append(float(np.abs(t).sum()))
    return np.array(ref), np.array(mag)


def solve_ref(m, K: int, S: int, shift: float, scale: float):
    """-> (b [S][K] z-basis solution, raw [S][K] coefficients of x^k, cond_inf(G), ||T||_inf) from the float64 moments m, exactly
    as given, in mpmath"""
    with mpmath.workdps(MP_DPS):
        m = [mpmath.mpf(float(v)) for v in np.asarray(m, dtype=np.float64)]
        G = mpmath.matrix(K, K)
        for j in range(K):
            for k in range(K):
                G[j, k] = m[j + k]
        Gi = G ** -1
        cond = mpmath.mnorm(G, "inf") * mpmath.mnorm(Gi, "inf")
        T = mpmath.matrix(K, K)
        sh, sc = mpmath.mpf(float(shift)), mpmath.mpf(float(scale))
        for k in range(K):
            for j in range(k + 1):
                T[j, k] = sc ** k * math.comb(k, j) * (-sh) ** (k - j)
        b = np.zeros((S, K))
        raw = np.zeros((S, K))
        for s in range(S):
            rhs = mpmath.matrix([m[(2 * K - 1) + s * K + k] for k in range(K)])
            bs = Gi * rhs
            rs = T * bs
            b[s] = [float(v) for v in bs]
            raw[s] = [float(v) for v in rs]
        return b, raw, float(cond), float(mpmath.mnorm(T, "inf"))


SPREADS = ("well", "clustered", "shifted")


def synthetic_moments(K: int, S: int, kind: str, n: int = 500, seed: int = 0):
    """(moments [(2K-1) + S K], shift, scale) of n sampled explanatory values x and S regressands:
    well      x uniform on [80, 120], shift 100, scale 1/20 (z on [-1, 1]);
    clustered x uniform on [85, 115], shift 50, scale 1/50 (z on [0.7, 1.3], far from 0: the monomials of z are nearly collinear,
              cond(G) up to ~1e12 at K = 6, still regular);
    shifted   x uniform on [80, 120], shift 60, scale 1/80 (z on [0.25, 0.75]: the back-transformation mixes every power)"""
    r = np.random.default_rng(1000 * K + 10 * S + SPREADS.index(kind) + 7 * seed)
    if kind == "clustered":
        x = r.uniform(85.0, 115.0, n)
        shift, scale = 50.0, 1.0 / 50.0
    else:
        x = r.uniform(80.0, 120.0, n)
        shift, scale = (100.0, 1.0 / 20.0) if kind == "well" else (60.0, 1.0 / 80.0)
    z = (x - shift) * scale
    Y = np.stack([np.maximum(x - 95.0 - 2.0 * s, 0.0) + r.normal(0.0, 1.0 + s, n) for s in range(S)])
    m, _ = moments_ref(z, Y, K)
    return m, shift, scale


def check_solution(raw, m, K, S, shift, scale, c, tag, z_basis=False, moment_err=1.0):
    """|raw - raw_ref|_inf <= c cond(G) eps ||T||_inf ||b_ref||_inf per state (z_basis: shift = 0, scale = 1 and T = I);
    moment_err: relative error of the moments themselves (1 for moments given exactly)"""
    b, ref, cond, tn = solve_ref(m, K, S, shift, scale)
    raw = np.asarray(raw, dtype=np.float64).reshape(S, K)
    for s in range(S):
        bound = c * cond * EPS * moment_err * tn * np.abs(b[s]).max()
        err = np.abs(raw[s] - ref[s]).max()
        assert err <= bound, (tag, s, err, bound, cond, raw[s], ref[s])
    return cond
