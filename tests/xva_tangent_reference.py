"""Numpy restatement of the DUAL bilateral xVA table: what mcx_tangent_xva (csrc/kt_book.hip kt_xva) should compute per path.

TEST INFRASTRUCTURE, built on tests/tangent_book_reference.py (DualBook, Dual, unsecured, thr), in float64 or long double.  Per
path, with c the counterparty, o the own name, x_m the dual unsecured exposure of metric date m, S_n = S_n(0, t_m) and
q_n = 1 - S_n(t_m, t_m+1) as dual atoms of the book, and the sums over m = 0 .. n_dates-2:

    cva = (1-R_c) sum pos(x_m) (S_c q_c)              dva = (1-R_o) sum neg(x_m) (S_o q_o)
    cva_ftd = (1-R_c) sum pos(x_m) ((S_c q_c) S_o)    dva_ftd = (1-R_o) sum neg(x_m) ((S_o q_o) S_c)      bcva = cva_ftd - dva_ftd

pos(x) = x where x.v > 0, neg(x) = -x where x.v < 0, both zero in value and tangents at x.v == 0 (torch.relu: the reference's tape,
and the convention of tangent_book_reference.cva).  A name given as None never defaults: S is the dual constant 1, q the dual
constant 0.  The products are associated as csrc/k4_xva.hip associates them: the weight S q first, then times the other name's S,
the loss given default at the end."""
import numpy as np

import tangent_book_reference as T

LD = np.longdouble
EVALUATIONS = ("cva", "dva", "cva_ftd", "dva_ftd", "bcva")
TERMS = np.array([3, 3, 4, 4, 4])          # factors of a date's summand, per record (the floor of the yardstick: 2^-52 (terms + 4))


def _images(x):
    return np.concatenate([x.v[None], x.d])


def xva(book, expo, rows, cp, own, threshold, recovery_c, recovery_o, collateralized=False, delayed=None, with_mag=False):
    """[5][1+NP][n] per path (records in EVALUATIONS order, image 0 the value).  book: the DualBook whose atoms the sides name;
    cp / own: (surv ids, cond ids) or None; expo [1+NP][rows][n] of one netting set.  with_mag: also the sum of the |summand| of
    every entry, image by image (for bcva: of both legs)"""
    dt = book.dtype
    zero = lambda: book.uniform(0.0)
    acc = [zero() for _ in range(4)]
    mag = np.zeros((5, 1 + book.NP, book.n), dtype=dt)

    def side(s, m):
        if s is None:
            return book.uniform(1.0), book.uniform(0.0)
        return book.atom(int(s[0][m])), 1.0 - book.atom(int(s[1][m]))

    for m in range(len(rows) - 1):
        x = T.unsecured(expo, int(rows[m]), threshold, collateralized, T._delayed(delayed, m), dt)
        up, dn = x.v > 0, x.v < 0
        ep = T.Dual(np.where(up, x.v, 0), np.where(up, x.d, 0))
        en = T.Dual(np.where(dn, -x.v, 0), np.where(dn, -x.d, 0))
        (Sc, qc), (So, qo) = side(cp, m), side(own, m)
        wc, wo = Sc * qc, So * qo
        terms = [ep * wc, en * wo, ep * (wc * So), en * (wo * Sc)]
        for r, t in enumerate(terms):
            acc[r] = acc[r] + t
            mag[r] += np.abs(_images(t))
    lgd = [dt(1.0) - dt(recovery_c), dt(1.0) - dt(recovery_o)]
    v = [acc[r] * lgd[r % 2] for r in range(4)]
    v.append(v[2] - v[3])
    for r in range(4):
        mag[r] *= abs(lgd[r % 2])
    mag[4] = mag[2] + mag[3]
    out = np.stack([_images(t) for t in v])
    return (out, mag) if with_mag else out


def sum_tolerance(t, bound):
    """of the sum over the paths of the per-path entries t [...][n]: n bound max|t| + n 2^-53 sum|t| (per-path error at the bound,
    plus the rounding of n additions in any order)"""
    t = np.abs(np.asarray(t, dtype=LD))
    n = t.shape[-1]
    return np.asarray(n * bound * t.max(axis=-1) + n * 2.0 ** -53 * t.sum(axis=-1), dtype=np.float64)
