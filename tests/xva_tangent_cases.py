"""Inputs of the dual xVA tests (tests/test_xva_tangent_host.py, tests/test_xva_tangent_kernels.py), all made on the host.

The book of tests/xva_cases.py (a payer swap under Vasicek + two CIR++ names) with a BilateralCVAMetric, compiled on the CPU oracle at
E metric dates (2: the smallest table with a summand; 11: the whole timeline) for its plan and its `_xva_atoms`; the regression's
coefficients perturbed as in tests/book_cases.py.  Paths, tangents and atom tangents are those of tangent_book_cases.inputs (quantised
so that x +- 2^-20 dx is exact).  The three unsecured modes are those of tangent_book_cases.metric_mode with the threshold scaled to
this book's exposures."""
import numpy as np

import book_cases as BC
import tangent_book_cases as TC
import tangent_book_reference as T
import xva_cases as xc
import xva_tangent_reference as XT
from mcx import _abi
from mcx.metrics.bcva_metric import BilateralCVAMetric

NP = _abi.TANGENT_NP
H = 2.0 ** -9                  # threshold of the thresholded and collateralised modes: of the size of the swap's exposures, exact in binary
DATES = (2, 11)
SIDES = ("both", "cp_none", "own_none")
GRID_CAP = 512                 # KT_XVA_GRID_CAP of csrc/kt_book.hip, in blocks of 256 paths (the host test reads it from the source)
K = 3


class Book:
    """the xva_cases book at E metric dates; the interface tangent_book_cases.inputs asks of a book"""

    def __init__(self, E, backend):
        sc = xc.controller(backend, [BilateralCVAMetric("cp", "own", xc.R_CP, xc.R_OWN)], n_main=1024, n_pre=BC.N_PRE, timeline=xc.TIMELINE[:E])
        sc.allow_fused = False
        sc.prepare()
        self.E, self.K, self.sc = E, sc.book_plan.n_basis, sc
        backend.book_set_coeffs(sc.book, 0, BC.perturbed_coeffs(sc, sc.book_plan.coeffs.copy()))
        self.plan, self.ev_param = sc.book_plan, None
        self.rows = sc.metric_exposure_indices.numpy().astype(np.int32)
        (cp, _rc), (own, _ro) = sc._xva_atoms[0]
        self.cp, self.own = tuple(np.array(a, dtype=np.int32) for a in cp), tuple(np.array(a, dtype=np.int32) for a in own)
        assert len(self.rows) == E and len(self.cp[0]) == E - 1

    def used_rows(self):
        a = self.plan.atoms
        return {(int(t), int(c)) for t, c in zip(a["t_idx"], a["col"]) if c >= 0}

    def sides(self, which):
        return {"both": (self.cp, self.own), "cp_none": (None, self.own), "own_none": (self.cp, None)}[which]


_BOOKS = {}


def book(E, backend):
    if E not in _BOOKS:
        _BOOKS[E] = Book(E, backend)
    return _BOOKS[E]


def metric_mode(mode, rows):
    """tangent_book_cases.metric_mode with this book's threshold"""
    threshold, coll, delayed = TC.metric_mode(mode, rows)
    return (H if threshold != 0.0 else 0.0), coll, delayed


def edges():
    """exact values planted in the value image of every exposure row: u == +-0, e == +-h, e just outside the band, both signs at the
    exposures' size"""
    return [0.0, H, -H, np.nextafter(H, np.inf), np.nextafter(-H, -np.inf), -0.0, 8.0 * H, -8.0 * H]


def plant(e, n, seed=7):
    """the edges into image 0 of expo e [1+NP][NS][rows][>= n] (netting set 0), in place -> the planted paths [n] (bool)"""
    rng = np.random.default_rng([seed, n])
    planted = np.zeros(n, dtype=bool)
    ed = edges()
    for r in range(e.shape[2]):
        at = rng.permutation(n)[:len(ed)]
        e[0, 0, r, at] = [ed[(k + r) % len(ed)] for k in range(len(at))]
        planted[at] = True
    return planted


def restated(b, x, host_expo, mode, which, with_mag=True):
    """{dtype: per-path [5][1+NP][n]}, magnitudes (long double) of the restatement on the exposures host_expo [1+NP][rows][n]"""
    threshold, coll, delayed = metric_mode(mode, b.rows)
    cp, own = b.sides(which)
    res, mag = {}, None
    for dt in (np.float64, T.LD):
        db = T.DualBook(b.plan, x.paths, x.dpaths, x.datoms, dtype=dt)
        res[dt], mag = XT.xva(db, host_expo, b.rows, cp, own, threshold, xc.R_CP, xc.R_OWN, coll, delayed, with_mag=True)
    return res, mag


def bounds(res, mag):
    """(yardstick per record [5], per-row bounds [5][1+NP]) from the restatement alone: 4 yardsticks, or the row's condition number
    times 2^-52 (terms + 4) where its entries cancel (tangent_book_reference.row_bounds)"""
    y = np.array([T.yardstick(res[np.float64][r], res[T.LD][r], XT.TERMS[r]) for r in range(5)])
    rb = np.stack([T.row_bounds(res[T.LD][r], mag[r], y[r], XT.TERMS[r]) for r in range(5)])
    return y, rb
