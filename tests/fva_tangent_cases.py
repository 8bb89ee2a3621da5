"""Inputs of the dual FVA tests (tests/test_fva_tangent_host.py, tests/test_fva_tangent_kernels.py), all made on the host.

The books, paths, tangents, modes and planted edges are those of tests/xva_tangent_cases.py (the xva_cases book at 2 and 11 metric
dates); FVA reads the S(0, t_m) atom list of each name (`sides(...)[k][0]`) and adds a fourth name choice, no name at all.  The
funding weights are those of tests/fva_reference.py's two curves on the case's timeline, next to a table of exact zeros, a negative
table and unit weights."""
import numpy as np

import fva_reference as fr
import fva_tangent_reference as FT
import tangent_book_reference as T
import xva_cases as xc
import xva_tangent_cases as XC

NP = XC.NP
DATES = XC.DATES
SIDES = ("both", "cp_none", "own_none", "none")
GRID_CAP = 1024                # KT_FVA_GRID_CAP of csrc/kt_book.hip, in blocks of 256 paths (the host test reads it from the source)
WEIGHTS = ("curves", "zero_lend", "negative", "unit")


def names(b, which):
    """(counterparty S ids | None, own S ids | None) of a name choice"""
    if which == "none":
        return None, None
    cp, own = b.sides(which)
    return (None if cp is None else cp[0]), (None if own is None else own[0])


def weights(E, kind="curves"):
    """(w_borrow, w_lend) [E-1] on the timeline of the book at E metric dates"""
    t = xc.TIMELINE[:E]
    wb, wl = fr.funding_weights(fr.BORROW_CURVE, t), fr.funding_weights(fr.LEND_CURVE, t)
    if kind == "zero_lend":
        wl = np.zeros(E - 1)
    elif kind == "negative":
        wb = -wb
    elif kind == "unit":
        wb, wl = np.ones(E - 1), np.ones(E - 1)
    else:
        assert kind == "curves"
    return wb, wl


def restated(b, x, host_expo, mode, which, kind="curves"):
    """{dtype: per-path [3][1+NP][n]}, magnitudes (long double) of the restatement on the exposures host_expo [1+NP][rows][n]"""
    threshold, coll, delayed = XC.metric_mode(mode, b.rows)
    cp, own = names(b, which)
    wb, wl = weights(b.E, kind)
    res, mag = {}, None
    for dt in (np.float64, T.LD):
        db = T.DualBook(b.plan, x.paths, x.dpaths, x.datoms, dtype=dt)
        res[dt], mag = FT.fva(db, host_expo, b.rows, cp, own, wb, wl, threshold, coll, delayed, with_mag=True)
    return res, mag


def bounds(res, mag):
    """(yardstick per record [3], per-row bounds [3][1+NP]) from the restatement alone: 4 yardsticks, or the row's condition number
    times 2^-52 (terms + 4) where its entries cancel (tangent_book_reference.row_bounds)"""
    y = np.array([T.yardstick(res[np.float64][r], res[T.LD][r], FT.TERMS[r]) for r in range(3)])
    rb = np.stack([T.row_bounds(res[T.LD][r], mag[r], y[r], FT.TERMS[r]) for r in range(3)])
    return y, rb


def sequential_legs(x_images):
    """x_images [E-1][1+NP][n], the dual unsecured exposures of the summand dates -> (fca, fba) [1+NP][n]: the sequential float64 sums
    over the dates of the exposure images where x.v > 0 and of their negatives where x.v < 0"""
    x = np.asarray(x_images, dtype=np.float64)
    fca, fba = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
    for m in range(x.shape[0]):
        fca = fca + np.where(x[m, 0] > 0, x[m], 0.0)
        fba = fba + np.where(x[m, 0] < 0, -x[m], 0.0)
    return fca, fba


def unsecured_images(b, host_expo, mode, dtype=np.float64):
    """[E-1][1+NP][n]: the dual unsecured exposure of every summand date"""
    threshold, coll, delayed = XC.metric_mode(mode, b.rows)
    out = []
    for m in range(b.E - 1):
        u = T.unsecured(host_expo, int(b.rows[m]), threshold, coll, T._delayed(delayed, m), dtype)
        out.append(np.concatenate([u.v[None], u.d]))
    return np.stack(out)
