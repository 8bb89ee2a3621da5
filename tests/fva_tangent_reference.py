"""Numpy restatement of the DUAL FVA table: what mcx_tangent_fva (csrc/kt_book.hip kt_fva) should compute per path.

TEST INFRASTRUCTURE, built on tests/tangent_book_reference.py (DualBook, Dual, unsecured), in float64 or long double.  Per path, with
c the counterparty, o the own name, x_m the dual unsecured exposure of metric date m, S_n = S_n(0, t_m) as dual atoms of the book,
the funding weights phi_b / phi_l as constants (no tangent) and the sums over m = 0 .. n_dates-2:

    w = S_c S_o        fca = sum pos(x_m) (w phi_b(m))        fba = sum neg(x_m) (w phi_l(m))        fva = fca - fba

pos(x) = x where x.v > 0, neg(x) = -x where x.v < 0, both zero in value and tangents at x.v == 0 (torch.relu: the reference's tape,
and the convention of tangent_book_reference.cva and xva_tangent_reference.xva).  A name given as None never defaults: S is the dual
constant 1.  The products are associated as csrc/k4_fva.hip associates them: w first, then w phi, then times the leg; the summand and
its addition to the accumulator are two roundings."""
import numpy as np

import tangent_book_reference as T
from xva_tangent_reference import sum_tolerance  # noqa: F401  (the tolerance of a full call's sums, shared with the xVA tests)

LD = np.longdouble
EVALUATIONS = ("fca", "fba", "fva")
TERMS = np.array([4, 4, 4])                # factors of a date's summand, per record (the floor of the yardstick: 2^-52 (terms + 4))


def _images(x):
    return np.concatenate([x.v[None], x.d])


def fva(book, expo, rows, cp_surv, own_surv, w_borrow, w_lend, threshold, collateralized=False, delayed=None, with_mag=False):
    """[3][1+NP][n] per path (records in EVALUATIONS order, image 0 the value).  book: the DualBook whose atoms the id lists name;
    cp_surv / own_surv: the S(0,t_m) atom ids [n_dates-1] or None; w_borrow / w_lend [n_dates-1]; expo [1+NP][rows][n] of one
    netting set.  with_mag: also the sum of the |summand| of every entry, image by image (for fva: of both legs)"""
    dt = book.dtype
    acc = [book.uniform(0.0), book.uniform(0.0)]
    mag = np.zeros((3, 1 + book.NP, book.n), dtype=dt)
    wb_t, wl_t = (np.asarray(w, dtype=np.float64).astype(dt) for w in (w_borrow, w_lend))
    for m in range(len(rows) - 1):
        x = T.unsecured(expo, int(rows[m]), threshold, collateralized, T._delayed(delayed, m), dt)
        up, dn = x.v > 0, x.v < 0
        ep = T.Dual(np.where(up, x.v, 0), np.where(up, x.d, 0))
        en = T.Dual(np.where(dn, -x.v, 0), np.where(dn, -x.d, 0))
        Sc = book.uniform(1.0) if cp_surv is None else book.atom(int(cp_surv[m]))
        So = book.uniform(1.0) if own_surv is None else book.atom(int(own_surv[m]))
        w = Sc * So
        wb, wl = w * wb_t[m], w * wl_t[m]
        for r, t in enumerate((ep * wb, en * wl)):
            acc[r] = acc[r] + t
            mag[r] += np.abs(_images(t))
    v = [acc[0], acc[1], acc[0] - acc[1]]
    mag[2] = mag[0] + mag[1]
    out = np.stack([_images(t) for t in v])
    return (out, mag) if with_mag else out
