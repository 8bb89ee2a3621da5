"""The dual Heston step maps (EULER, heston.py:109-121; Andersen QE, :161-253 of the reference) restated in numpy with explicit
tangents, in float64 or np.longdouble.  Plain numpy: no torch, nothing of the library under test.

A dual number is a value row [n] and a tangent block [P][n].  The subgradients are torch's, since they decide the reference's
numbers: torch.clamp passes the gradient on the closed side(s), a hard degree of truth has none, and sqrt keeps a zero tangent zero
where 1 / (2 sqrt(x)) is infinite (torch.clamp's backward discards it with a `where`).  The operations are the reference's own —
true divisions, sqrt(2 / psi) * sqrt(t) as two roots — not the kernels' grouped reciprocals; tests/step_reference.py `_heston` is
the primal this follows.

`dual_paths` takes exactly the doubles a kernel gets: the descriptor tables (slot parameters, initial state, per-step constants,
the factor) and their tangents [...][P], the schedule, the normals and the uniforms.  It returns paths [T][2][n], tangents
[P][T][2][n] and the MARGINS of the draws, each a minimum over all path-steps: a device whose exp / log / reciprocal differ from
numpy's by ulps takes the same masks as long as every margin is far above rounding."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

EPS = 1e-12
MARGIN = 1e-9


class Dual:
    __slots__ = ("v", "d")
    __array_ufunc__ = None                   # numpy operands defer to the reflected operators below

    def __init__(self, v, d):
        self.v, self.d = v, d

    @staticmethod
    def const(v, like):
        return Dual(np.broadcast_to(np.asarray(v, dtype=like.v.dtype), like.v.shape).copy(), np.zeros_like(like.d))

    def _lift(self, o):
        return o if isinstance(o, Dual) else Dual.const(o, self)

    def __add__(self, o):
        o = self._lift(o)
        return Dual(self.v + o.v, self.d + o.d)

    __radd__ = __add__

    def __sub__(self, o):
        o = self._lift(o)
        return Dual(self.v - o.v, self.d - o.d)

    def __rsub__(self, o):
        return self._lift(o) - self

    def __mul__(self, o):
        o = self._lift(o)
        return Dual(self.v * o.v, self.d * o.v + self.v * o.d)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._lift(o)
        q = self.v / o.v
        return Dual(q, (self.d - q * o.d) / o.v)

    def __rtruediv__(self, o):
        return self._lift(o) / self


def dsqrt(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(a.v)
        d = np.where(a.d == 0, a.d.dtype.type(0), a.d / (2 * r))
    return Dual(r, d)


def dlog(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return Dual(np.log(a.v), a.d / a.v)


def dclamp(a, lo=None, hi=None):
    """torch.clamp: the gradient passes iff lo <= x <= hi; a NaN value stays NaN"""
    v, ok = a.v, np.ones(a.v.shape, dtype=bool)
    if lo is not None:
        ok &= a.v >= lo
        v = np.where(v < lo, v.dtype.type(lo), v)
    if hi is not None:
        ok &= a.v <= hi
        v = np.where(v > hi, v.dtype.type(hi), v)
    return Dual(v, np.where(ok, a.d, a.d.dtype.type(0)))


def ddegree(x, fuzzy, eps):
    """maths/maths.py compute_degree_of_truth: clamp((x + eps) / (2 eps), 0, 1), or the hard indicator without a gradient"""
    if not fuzzy:
        return Dual(np.where(x.v > 0, x.v.dtype.type(1), x.v.dtype.type(0)), np.zeros_like(x.d))
    return dclamp((x + eps) / (2 * eps), 0.0, 1.0)


def _band(x, fuzzy, eps):
    """distance of x from the edges of its fuzzy band, or from 0 when the indicator is hard"""
    x = np.asarray(x, dtype=np.float64)
    return float(np.min(np.minimum(np.abs(x + eps), np.abs(x - eps)))) if fuzzy else float(np.min(np.abs(x)))


def tables_of(plan, d0, dd, fuzzy):
    """what `dual_paths` reads, from a SimPlan and the descriptor blocks / tangents of aad.descriptor_tangents (dd[...][P])"""
    return SimpleNamespace(qe=plan.scheme.name == "QE", fuzzy=bool(fuzzy), dt=np.array(plan.steps["dt"]), sqrt_dt=np.array(plan.steps["sqrt_dt"]),
                           store_idx=np.array(plan.steps["store_idx"]), n_initial_store=plan.n_initial_store, n_dates=plan.n_dates,
                           slots=d0["slots"][0], dslots=dd["slots"][0], init=d0["init"], dinit=dd["init"], aux=d0["aux"][:, 0], daux=dd["aux"][:, 0],
                           chol=d0["chol"][0], dchol=dd["chol"][0])


def dual_paths(tb, z, u=None, dtype=np.float64):
    """z [n_steps][2][n], u [n_steps][n] (QE).  -> paths [T][2][n], dpaths [P][T][2][n] in `dtype`, margins (dict of floats + finite)"""
    z = np.asarray(z, dtype=dtype)
    n, P = z.shape[2], tb.dslots.shape[-1]
    T = dtype

    def scalar(v, dv):
        return Dual(np.full(n, T(v), dtype=dtype), np.repeat(np.asarray(dv, dtype=dtype)[:, None], n, axis=1))

    par = [scalar(tb.slots[j], tb.dslots[j]) for j in range(8)]
    sigma, rate, kappa, theta = par[1], par[2], par[4], par[5]
    logS, v = scalar(tb.init[0], tb.dinit[0]), scalar(tb.init[1], tb.dinit[1])
    paths, dpaths = np.zeros((tb.n_dates, 2, n), dtype=dtype), np.zeros((P, tb.n_dates, 2, n), dtype=dtype)

    def store(t):
        paths[t, 0], paths[t, 1], dpaths[:, t, 0], dpaths[:, t, 1] = logS.v, v.v, logS.d, v.d

    for t in range(tb.n_initial_store):
        store(t)
    mar = dict(psi=np.inf, u=np.inf, v=np.inf, psi_eps=np.inf, kinks=np.inf, in_band_psi=0, in_band_u=0)
    for k in range(len(tb.dt)):
        dt, sq, z0, z1 = T(tb.dt[k]), T(tb.sqrt_dt[k]), z[k, 0], z[k, 1]
        if not tb.qe:                                                           # heston.py:109-121; corr_randn = z @ L.T with a dual L
            l10, l11 = scalar(tb.chol[1, 0], tb.dchol[1, 0]), scalar(tb.chol[1, 1], tb.dchol[1, 1])
            zc1 = l10 * z0 + l11 * z1
            mar["v"] = min(mar["v"], float(np.min(np.abs(v.v))))
            sv = dsqrt(dclamp(v, 0.0))
            logS_n = logS + (rate - 0.5 * v) * dt + sv * sq * z0
            v_raw = v + kappa * (theta - v) * dt + sigma * sv * sq * zc1
            mar["v"] = min(mar["v"], float(np.min(np.abs(v_raw.v))))
            logS, v = logS_n, dclamp(v_raw, 0.0)
        else:                                                                   # heston.py:161-253
            ax = [scalar(tb.aux[k, e], tb.daux[k, e]) for e in range(8)]
            E, K0, K1, K2, K3, K4, c1, c2 = ax
            uk = np.asarray(u[k], dtype=dtype)
            m = theta + (v - theta) * E
            s2 = v * c1 + c2
            psi = s2 / (m * m + EPS)
            invpsi = 1.0 / (psi + EPS)
            tm1 = 2.0 * invpsi - 1.0
            t_ = dclamp(tm1, 0.0)
            b2 = dclamp(tm1 + dsqrt(2.0 * invpsi) * dsqrt(t_), 0.0)
            b = dsqrt(b2)
            a = m / (1.0 + b2)
            bz = b + z1
            v1 = a * (bz * bz)
            p_raw = (psi - 1.0) / (psi + 1.0)
            p = dclamp(p_raw, 0.0, 1.0 - 1e-6)
            beta = (1.0 - p) / (m + EPS)
            omu = np.maximum(T(1.0) - uk, T(EPS))
            omp = dclamp(1.0 - p, EPS)
            v_tail = dlog(omp / omu) / (beta + EPS)
            mu = uk - p
            w_mass = ddegree(mu, tb.fuzzy, 0.3)
            psi_m = psi - 1.5
            w = ddegree(psi_m, tb.fuzzy, 0.5)
            vn = (1.0 - w) * v1 + w * (w_mass * v_tail)
            var_int = dclamp(K3 * v + K4 * vn, 0.0)
            vol = dsqrt(dclamp(var_int, EPS))
            logS = logS + rate * dt + K0 + K1 * v + K2 * vn + vol * z0
            v = vn
            mar["psi"] = min(mar["psi"], _band(psi_m.v, tb.fuzzy, 0.5))
            mar["u"] = min(mar["u"], _band(mu.v, tb.fuzzy, 0.3))
            mar["psi_eps"] = min(mar["psi_eps"], float(np.min(np.abs(psi.v + EPS))))
            if tb.fuzzy:                     # path-steps strictly inside a fuzzy band: there the indicator carries gradient
                mar["in_band_psi"] += int(np.sum(np.abs(np.asarray(psi_m.v, dtype=np.float64)) < 0.5))
                mar["in_band_u"] += int(np.sum(np.abs(np.asarray(mu.v, dtype=np.float64)) < 0.3))
            # the other clamps of the step whose mask could flip: t at 2 / psi = 1, p at psi = 1 and at its cap
            mar["kinks"] = min(mar["kinks"], float(np.min(np.abs(tm1.v))), float(np.min(np.abs(p_raw.v))), float(np.min(np.abs(p_raw.v - (1.0 - 1e-6)))))
        if tb.store_idx[k] >= 0:
            store(int(tb.store_idx[k]))
    mar["finite"] = bool(np.isfinite(paths).all() and np.isfinite(dpaths).all())
    return paths, dpaths, mar


def margins_hold(mar) -> bool:
    """the keep condition of the fixtures and of the kernel tests' inputs: nothing non-finite, every margin above MARGIN"""
    return mar["finite"] and all(mar[key] > MARGIN for key in ("psi", "u", "v", "psi_eps", "kinks"))


def rounding_gap(a, b):
    """largest |a - b| over a row (all paths of one image, date and state variable), relative to the row's largest |b|; rows that are
    zero in b must be zero in a"""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    scale = np.abs(b).max(axis=-1, keepdims=True)
    gap = np.abs(a - b).max(axis=-1, keepdims=True)
    assert not gap[scale == 0].any()
    return float((gap / np.where(scale == 0, 1, scale)).max())
