"""Plain numpy restatements of what the metric kernels (csrc/k4_reduce.hip, csrc/k5_select.hip) compute.

TEST INFRASTRUCTURE: no GPU, no oracle.  Every function states the OPERATION, not the kernel's algorithm: sums are exact
(math.fsum over exactly representable terms), histograms are np.bincount over the order-preserving key, the bracket pass is a
boolean mask and a sort.  tests/test_metric_kernels.py first pins these to the CPU oracle and then the kernels to these."""
from __future__ import annotations

import itertools
import math

import numpy as np

SIGN = np.uint64(1 << 63)


# ---- netting-set post-processing (dev_thr / dev_unsec of mcx_internal.h) ---------------------------------------------------------
def thr_np(x: np.ndarray, h: float) -> np.ndarray:
    """x beyond the threshold band [-h, h], 0 inside it; h == 0 leaves x (and a NaN) untouched, h != 0 maps a NaN to 0"""
    x = np.asarray(x, dtype=np.float64)
    if h == 0.0:
        return x.copy()
    with np.errstate(invalid="ignore"):
        return np.where(x > h, x - h, np.where(x < -h, x + h, 0.0))


def unsecured_np(x: np.ndarray, rows, delayed, h: float, collateralized: bool) -> np.ndarray:
    """x [matrix rows][n] -> [len(rows)][n]: thr(x[row]) uncollateralised; x[row] - thr(x[delayed]) (0 where delayed is -1 or
    absent) collateralised"""
    x = np.asarray(x, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    e = x[rows]
    if not collateralized:
        return thr_np(e, h)
    coll = np.zeros_like(e)
    if delayed is not None:
        d = np.asarray(delayed, dtype=np.int64)
        ok = d >= 0
        coll[ok] = thr_np(x[d[ok]], h)
    with np.errstate(invalid="ignore"):
        return e - coll


def relu_parts(u: np.ndarray):
    """(max(u, 0), min(u, 0)) with a NaN counted as 0 on both sides (fmax / fmin of the device, `x > 0 ? x : 0` of the oracle)"""
    with np.errstate(invalid="ignore"):
        return np.where(u > 0.0, u, 0.0), np.where(u < 0.0, u, 0.0)


# ---- radix select -----------------------------------------------------------------------------------------------------------------
def key_np(x: np.ndarray) -> np.ndarray:
    """order-preserving uint64 image of a double (dev_key): negative -> all bits flipped, else the sign bit set"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where((b & SIGN) != 0, ~b, b | SIGN)


def key_to_double_np(k: np.ndarray) -> np.ndarray:
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where((k & SIGN) != 0, k & ~SIGN, ~k).astype(np.uint64).view(np.float64)


def hist_np(u: np.ndarray, prefix: np.ndarray, shift: int, bits: int, row_n=None) -> np.ndarray:
    """u [E][n] values, prefix [E][n_sel] uint64 -> [E][n_sel][2^bits] int64: per date and selection the elements whose key agrees
    with the prefix above bit shift + bits, binned by the digit (key >> shift) & (2^bits - 1).  shift + bits == 64 matches every
    element.  row_n: only the first min(row_n[m], n) elements of row m take part."""
    k = key_np(u)
    E, n = k.shape
    prefix = np.asarray(prefix, dtype=np.uint64).reshape(E, -1)
    nb, hi = 1 << bits, shift + bits
    digit = ((k >> np.uint64(shift)) & np.uint64(nb - 1)).astype(np.int64)
    top = k >> np.uint64(hi) if hi < 64 else None
    live = np.ones((E, n), dtype=bool) if row_n is None else np.arange(n)[None, :] < np.asarray(row_n, dtype=np.int64)[:, None]
    cell = digit + (np.arange(E, dtype=np.int64) * nb)[:, None]          # one bincount over all dates: bin + date * nb
    out = np.zeros((E, prefix.shape[1], nb), dtype=np.int64)
    for j in range(prefix.shape[1]):
        match = live if hi >= 64 else live & (top == (prefix[:, j] >> np.uint64(hi))[:, None])
        out[:, j] = np.bincount(cell[match], minlength=E * nb).reshape(E, nb)
    return out


def narrow_np(hist: np.ndarray, prefix: np.ndarray, rem: np.ndarray, shift: int):
    """the cumulative-count rule of one digit: b = #{bins whose inclusive cumulative count <= rem}; the prefix gains b << shift and
    rem loses the count below bin b.  hist [...][nb], prefix uint64 [...], rem int64 [...] -> (prefix, rem)"""
    cum = np.cumsum(np.asarray(hist, dtype=np.int64), axis=-1)
    rem = np.asarray(rem, dtype=np.int64)
    b = (cum <= rem[..., None]).sum(axis=-1)
    below = np.where(b > 0, np.take_along_axis(cum, np.maximum(b - 1, 0)[..., None], axis=-1)[..., 0], 0)
    return np.asarray(prefix, dtype=np.uint64) | (b.astype(np.uint64) << np.uint64(shift)), rem - below


def bracket_np(u: np.ndarray, lo, hi):
    """per date m: (#{x < lo[m]}, sorted values with lo[m] <= x <= hi[m]); a NaN is neither below nor inside"""
    out = []
    for m in range(u.shape[0]):
        with np.errstate(invalid="ignore"):
            below = int((u[m] < lo[m]).sum())
            inside = np.sort(u[m][(u[m] >= lo[m]) & (u[m] <= hi[m])])
        out.append((below, inside))
    return out


# ---- accumulator records ------------------------------------------------------------------------------------------------------------
def _split(d: np.ndarray):
    """Veltkamp split d = hi + lo with 26-bit halves: hi*hi, 2*hi*lo and lo*lo are then exact doubles"""
    c = 134217729.0 * d
    hi = c - (c - d)
    return hi, d - hi


def acc_exact(v: np.ndarray):
    """the record (n, shift, s1, s2) of a vector as the kernels define it, with exact sums: shift = v[0], d = fl(v - v[0]) (the
    one rounding the device makes too), s1 = sum d and s2 = sum d^2 by math.fsum over exactly representable terms (each d^2 as
    the three exact products of its Veltkamp halves).  Also returns sum |d| for the summation-error bounds."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    n = v.shape[0]
    if n == 0:
        return dict(n=0.0, shift=0.0, s1=0.0, s2=0.0, abs1=0.0)
    d = v - v[0]
    hi, lo = _split(d)
    terms = itertools.chain((hi * hi).tolist(), (2.0 * hi * lo).tolist(), (lo * lo).tolist())
    return dict(n=float(n), shift=float(v[0]), s1=math.fsum(d.tolist()), s2=math.fsum(terms), abs1=math.fsum(np.abs(d).tolist()))


def mean_err_longdouble(v: np.ndarray):
    """two-pass mean, unbiased std / sqrt(n) and M2 in long double"""
    x = np.asarray(v, dtype=np.longdouble)
    n = x.shape[0]
    mean = x.sum() / n
    r = x - mean
    m2 = (r * r).sum() - r.sum() ** 2 / n
    err = np.sqrt(m2 / (n - 1)) / np.sqrt(np.longdouble(n)) if n > 1 else np.longdouble("nan")
    return float(mean), float(err), float(m2)
