"""kt_xva (csrc/kt_book.hip) through the C ABI, mcx_tangent_xva: per path and per parameter slot against the long-double restatement of
tests/xva_tangent_reference.py, which tests/test_xva_tangent_host.py validates on the host.

Inputs are those of tests/xva_tangent_cases.py: the xva_cases book compiled on the CPU oracle at 2 and 11 metric dates (the device
book is created from the same plan), host-made paths, tangents and atom tangents at 1, 255 and 257 paths in tensors with a padded
leading dimension, NaN in the pad and in every (date, state) row no atom names.  The exposures are mcx_tangent_eval's output with exact
edges planted in the value image of every row: +-0.0, +-h, the neighbours of +-h outside the band, +-8h.

Per-path bound.  One-path calls on column i of the padded tensors give the per-path records [5][1+NP][n].  A gap is |device -
long-double restatement| relative to the largest |entry| of the row (one image of one record over the paths).  The yardstick of a
record is the same gap between the restatement's float64 run and its long-double run, floored at 2^-52 (terms + 4), 3 terms for cva /
dva and 4 for the first-to-default forms and bcva; the bound is 4 yardsticks.  A row that cancels between the dates or between the
legs (the tangents, bcva, any row at one path) is held to its condition number instead (tangent_book_reference.row_bounds).  The sums
of a full call are held to n bound max|t| + n 2^-53 sum|t| over the restatement's summands t.  Nothing is taken from the device.

Measured on the MI355X (yardstick / device gap / bound of the row closest to its bound, the census this module prints with `pytest -s`;
README.md, "Forward-mode xVA"):
  cva, cva_ftd        1.30e-14 / 1.31e-14 / 5.20e-14   255 paths, 11 dates, collateralised
  dva, dva_ftd, bcva  1.33e-14 / 1.43e-14 / 5.30e-14   one path, 11 dates, collateralised
  sums                at most 0.27 of their tolerance; 2.0e-6 of it at 131,329 paths (1.7e-8 against the two halves)
  means               sum / n against mcx_reduce_xva's mean: at most 0.0033 of the same tolerance over n, all three side choices
No row of any case needed its condition number.  The workspace refusal cannot be reached through the entry point (512 x 25 partials
always fit the handle's 8 MiB workspace and 1 MiB pinned buffer), so it is not among the refusals tested."""
import ctypes as C

import numpy as np
import pytest
import torch

import tangent_book_cases as TC
import tangent_book_reference as T
import xva_cases as xc
import xva_tangent_cases as XC
import xva_tangent_reference as XT
from mcx import _abi
from mcx._native import McxError
from mcx.plan import UnsecuredSpec

pytestmark = pytest.mark.gpu
NP = TC.NP
LD = np.longdouble
MODES = TC.MODES
WORST = {}                     # record -> (gap / bound, yardstick, gap, bound, case) of the row closest to its bound
_CASES = {}


@pytest.fixture(scope="module")
def dbook(hip, oracle):
    made = {}

    def get(E):
        if E not in made:
            made[E] = hip.book_create(XC.book(E, oracle).plan)
        return made[E]
    yield get
    made.clear()
    _CASES.clear()


def _nan(hip, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=hip.device)


class _Case:
    """the inputs of (E, n) on the device (leading dimension ld, NaN in the pad) and the planted exposures on both sides"""

    def __init__(self, hip, oracle, book, E, n):
        b = XC.book(E, oracle)
        x = TC.inputs(b, n, oracle)
        self.b, self.x, self.n, self.ld = b, x, n, TC.ld_of(n)
        self.paths, self.dpaths = hip.from_numpy(TC.padded(x.paths, self.ld)), hip.from_numpy(TC.padded(x.dpaths, self.ld))
        self.datoms = hip.from_numpy(x.datoms)
        plan = b.plan
        cfs, expo = _nan(hip, 1 + NP, plan.n_netting_sets, self.ld), _nan(hip, 1 + NP, plan.n_netting_sets, int(plan.n_expo_rows), self.ld)
        hip.tangent_eval(book, self.datoms, hip.from_numpy(x.coeffs), hip.from_numpy(x.dcoeffs), self.paths, self.dpaths, n_paths=n, out=(cfs, expo))
        e = expo.cpu().numpy()
        self.planted = XC.plant(e, n)
        e[..., n:] = np.nan
        self.e = e
        self.expo = hip.from_numpy(e)
        self.host = e[:, 0, :, :n]


def _case(hip, oracle, dbook, E, n):
    if (E, n) not in _CASES:
        _CASES[E, n] = _Case(hip, oracle, dbook(E), E, n)
    return _CASES[E, n]


def _call(hip, book, c, mode, which, lo=0, hi=None, expo=None, datoms=None, dpaths=None, swap=False, out=None):
    """mcx_tangent_xva on the paths [lo, hi) of the case, as path slices of the padded tensors"""
    hi = c.n if hi is None else hi
    threshold, coll, delayed = XC.metric_mode(mode, c.b.rows)
    cp, own = c.b.sides(which)
    rc_, ro_ = xc.R_CP, xc.R_OWN
    if swap:
        cp, own, rc_, ro_ = own, cp, ro_, rc_
    expo = c.expo if expo is None else expo
    dpaths = c.dpaths if dpaths is None else dpaths
    return hip.tangent_xva(book, c.datoms if datoms is None else datoms, c.b.rows, cp, rc_, own, ro_, threshold, expo[..., lo:hi], 0,
                           c.paths[:, :, lo:hi], dpaths[..., lo:hi], delayed, coll, out=out)


def _note(r, y, gap, bound, case):
    name = XT.EVALUATIONS[r]
    if name not in WORST or gap / bound > WORST[name][0]:
        WORST[name] = (gap / bound, y, gap, bound, case)


@pytest.mark.parametrize("which", XC.SIDES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("E", XC.DATES)
@pytest.mark.parametrize("n", TC.SIZES)
def test_xva_against_the_restatement(n, E, mode, which, hip, oracle, dbook):
    book, c = dbook(E), _case(hip, oracle, dbook, E, n)
    b = c.b
    threshold, coll, delayed = XC.metric_mode(mode, b.rows)
    res, mag = XC.restated(b, c.x, c.host, mode, which)
    y, rb = XC.bounds(res, mag)
    hi = res[LD]
    if coll:        # e - thr(d) is rounded before its sign is read: off the planted paths the difference is exactly 0 or far from 0
        for m in range(E - 1):
            if delayed[m] >= 0:
                a_ = c.host[0, b.rows[m]].astype(LD)
                c_ = T.thr(T.Dual(c.host[0, delayed[m]].astype(LD), c.host[1:, delayed[m]].astype(LD)), LD(threshold)).v
                free = ~c.planted & ~((a_ == 0) & (c_ == 0))
                assert (np.abs(a_ - c_)[free] > T.TIE_FACTOR * 4.0 * y.max() * (np.abs(a_) + np.abs(c_))[free]).all(), (mode, n, m)
    if n >= 255:                                                               # both signs of unsecured exposure on every metric date
        for m in range(E - 1):
            u = T.unsecured(c.host, int(b.rows[m]), threshold, coll, -1 if delayed is None else int(delayed[m])).v
            assert (u > 0).any() and (u < 0).any(), (mode, m)
    # per path: one-path calls on column i
    got = np.stack([_call(hip, book, c, mode, which, i, i + 1) for i in range(n)], axis=-1)         # [5][1+NP][n]
    assert not np.isnan(got).any()
    case = f"n={n} E={E} {mode} {which}"
    for r in range(5):
        gaps = T.row_gaps(got[r], hi[r])
        k = int(np.argmax(gaps / rb[r]))
        print(f"xva {XT.EVALUATIONS[r]} {case}: yardstick {y[r]:.3e}, device gap {gaps[k]:.3e}, bound {rb[r][k]:.3e}"
              f" ({int((rb[r] > 4.0 * y[r]).sum())} of {1 + NP} rows held to their condition number)")
        _note(r, y[r], float(gaps[k]), float(rb[r][k]), case)
        assert (gaps <= rb[r]).all(), (case, XT.EVALUATIONS[r], gaps, rb[r])
    if n > 1:
        assert np.abs(hi[4, 1:]).max() > 0 and np.abs(hi[:, 0]).max() > 0
    # the sums of the full call
    sums = _call(hip, book, c, mode, which)
    tol = _sum_tol(hi, rb, n)
    want = hi.sum(axis=-1)
    gap = np.abs(sums.astype(LD) - want).astype(np.float64)
    print(f"xva sums {case}: worst gap / tolerance {float(np.max(gap / np.where(tol > 0, tol, 1))):.3e}")
    assert (gap <= tol).all(), (case, gap, tol)
    # the value sums over the paths, divided by n, are the means of mcx_reduce_xva on the same sides, at the sum bound (a record of
    # a name that never defaults is an exact zero on both sides: tolerance 0)
    cp, own = b.sides(which)
    spec = UnsecuredSpec(b.rows, delayed, threshold, coll)
    rec = hip.reduce_xva(book, spec, cp, xc.R_CP, own, xc.R_OWN, c.expo[0, 0][:, :n], c.paths[:, :, :n])
    mean = rec["shift"] + rec["s1"] / rec["n"]
    mgap, mtol = np.abs(sums[:, 0] / n - mean), tol[:, 0] / n
    print(f"xva means {case}: worst |sum / n - mcx_reduce_xva mean| / tolerance {float(np.max(mgap / np.where(mtol > 0, mtol, 1))):.3e}")
    assert (mgap <= mtol).all(), (case, sums[:, 0] / n, mean, mtol)


def _sum_tol(hi, rb, n):
    """of the sums [5][1+NP] over the n paths, every row at its own per-path bound"""
    return np.stack([XT.sum_tolerance(hi[r], rb[r]) for r in range(5)])


def test_past_the_first_grid_stride_round(hip, oracle, dbook):
    """cap x 256 + 257 paths at 2 metric dates: the second round of the grid stride adds into the lanes' sums"""
    n = TC.stride_size(XC.GRID_CAP)
    book, c = dbook(2), _Case(hip, oracle, dbook(2), 2, n)
    mode, which = "thresholded", "both"
    res, mag = XC.restated(c.b, c.x, c.host, mode, which)
    y, rb = XC.bounds(res, mag)
    tol = _sum_tol(res[LD], rb, n)
    sums = _call(hip, book, c, mode, which)
    half = n // 2
    halves = _call(hip, book, c, mode, which, 0, half) + _call(hip, book, c, mode, which, half, n)
    want = res[LD].sum(axis=-1)
    g1, g2 = np.abs(sums.astype(LD) - want).astype(np.float64), np.abs(sums - halves)
    print(f"xva grid stride n={n}: worst gap / tolerance {float(np.max(g1 / tol)):.3e} (restatement), {float(np.max(g2 / tol)):.3e} (halves)")
    assert (g1 <= tol).all() and (g2 <= tol).all()
    assert sums.tobytes() == _call(hip, book, c, mode, which).tobytes()


@pytest.mark.parametrize("mode", ["unthresholded", "collateralised"])
def test_device_identities(mode, hip, oracle, dbook):
    n, E = 257, 11
    book, c = dbook(E), _case(hip, oracle, dbook, E, n)
    both = _call(hip, book, c, mode, "both")
    assert both.tobytes() == _call(hip, book, c, mode, "both").tobytes()                 # two calls: identical bytes
    assert (both[:4, 0] > 0).all() and np.abs(both[:, 1:]).min() > 0
    # a name that never defaults
    own0, cp0 = _call(hip, book, c, mode, "own_none"), _call(hip, book, c, mode, "cp_none")
    assert (own0[[1, 3]] == 0.0).all() and own0[2].tobytes() == own0[0].tobytes() and own0[4].tobytes() == own0[2].tobytes()
    assert (cp0[[0, 2]] == 0.0).all() and cp0[3].tobytes() == cp0[1].tobytes() and (cp0[4] == -cp0[3]).all()
    assert own0[0].tobytes() == both[0].tobytes() and cp0[1].tobytes() == both[1].tobytes()
    # names swapped and every exposure image negated: the legs change places, bcva changes sign, bit for bit in every image
    neg = hip.from_numpy(-c.e)
    sw = _call(hip, book, c, mode, "both", expo=neg, swap=True)
    assert sw[0].tobytes() == both[1].tobytes() and sw[1].tobytes() == both[0].tobytes()
    assert sw[2].tobytes() == both[3].tobytes() and sw[3].tobytes() == both[2].tobytes()
    assert sw[4].tobytes() == (-both[4]).tobytes()
    # a zero tangent slot gives exact zeros in that slot and leaves the others' bytes
    q = 2
    dat, dp, ex = c.x.datoms.copy(), TC.padded(c.x.dpaths, c.ld), c.e.copy()
    dat[:, :, q], dp[q, ..., :n], ex[1 + q, ..., :n] = 0.0, 0.0, 0.0
    z = _call(hip, book, c, mode, "both", expo=hip.from_numpy(ex), datoms=hip.from_numpy(dat), dpaths=hip.from_numpy(dp))
    assert (z[:, 1 + q] == 0.0).all()
    keep = [k for k in range(1 + NP) if k != 1 + q]
    assert z[:, keep].tobytes() == both[:, keep].tobytes()
    # every tangent input times 2: the tangent sums double exactly, the value sums keep their bytes
    ex2 = c.e.copy()
    ex2[1:] *= 2.0
    d2 = _call(hip, book, c, mode, "both", expo=hip.from_numpy(ex2), datoms=hip.from_numpy(2.0 * c.x.datoms),
               dpaths=hip.from_numpy(2.0 * TC.padded(c.x.dpaths, c.ld)))
    assert d2[:, 0].tobytes() == both[:, 0].tobytes() and d2[:, 1:].tobytes() == (2.0 * both[:, 1:]).tobytes()


def _raw(hip, book, c, mode, **over):
    """the entry point itself with one argument replaced -> (status, the poisoned output)"""
    threshold, coll, delayed = XC.metric_mode(mode, c.b.rows)
    out = np.full((5, 1 + NP), 777.0)
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
    a = dict(rows=i32(c.b.rows), delayed=i32(delayed), sc=i32(c.b.cp[0]), cc=i32(c.b.cp[1]), so=i32(c.b.own[0]), co=i32(c.b.own[1]),
             n=c.n, ld=c.ld, E=len(c.b.rows), out=out, handle=hip.h, book_ptr=book.ptr)
    a.update(over)
    vp = lambda t: C.c_void_p(t.data_ptr())
    rc = hip.lib.mcx_tangent_xva(a["handle"], a["book_ptr"], vp(c.datoms), _abi.ptr(a["rows"]), _abi.ptr(a["delayed"]), C.c_int32(int(coll)),
                                 C.c_int32(a["E"]), C.c_double(threshold), _abi.ptr(a["sc"]), _abi.ptr(a["cc"]), C.c_double(xc.R_CP),
                                 _abi.ptr(a["so"]), _abi.ptr(a["co"]), C.c_double(xc.R_OWN), vp(c.expo[0, 0]), C.c_int64(c.expo.stride(0)),
                                 vp(c.paths), vp(c.dpaths), C.c_int64(a["n"]), C.c_int64(a["ld"]), C.c_int32(c.paths.shape[0]),
                                 _abi.ptr(a["out"]), hip._stream())
    return rc, out


def test_refusals_leave_the_output_untouched_and_empty_calls_give_zeros(hip, oracle, dbook):
    n, E = 257, 11
    book, c = dbook(E), _case(hip, oracle, dbook, E, n)
    b = c.b
    n_atoms, n_rows = len(b.plan.atoms), int(b.plan.n_expo_rows)
    ok_rc, ok = _raw(hip, book, c, "collateralised")
    assert ok_rc == 0 and ok.tobytes() == _call(hip, book, c, "collateralised", "both").tobytes()

    def bad(ids, k, v):
        out = np.array(ids, dtype=np.int32)
        out[k] = v
        return out
    _, _, delayed = XC.metric_mode("collateralised", b.rows)
    refusals = [
        ("atom out of range", dict(sc=bad(b.cp[0], 3, n_atoms))), ("atom out of range", dict(cc=bad(b.cp[1], 0, -1))),
        ("atom out of range", dict(so=bad(b.own[0], E - 2, n_atoms))), ("atom out of range", dict(co=bad(b.own[1], 1, n_atoms + 5))),
        ("exposure row", dict(rows=bad(b.rows, 2, n_rows))), ("exposure row", dict(rows=bad(b.rows, E - 1, -1))),
        ("exposure row", dict(delayed=bad(delayed, 4, n_rows))),
        ("leading dimension", dict(ld=n - 1)),
        ("both or neither", dict(cc=None)), ("both or neither", dict(so=None)),
    ]
    for text, over in refusals:
        rc, out = _raw(hip, book, c, "collateralised", **over)
        assert rc == -2 and (out == 777.0).all(), (text, over, rc)
        assert text in hip.lib.mcx_last_error(hip.h).decode(), (text, hip.lib.mcx_last_error(hip.h))
    for over in (dict(handle=None), dict(book_ptr=None), dict(rows=None), dict(out=None)):
        rc, out = _raw(hip, book, c, "collateralised", **over)
        assert rc == -1 and (out == 777.0).all(), over
    with pytest.raises(McxError) as e:                                          # the binding raises what the library refuses
        hip.tangent_xva(book, c.datoms, bad(b.rows, 0, n_rows), b.cp, xc.R_CP, b.own, xc.R_OWN, 0.0, c.expo, 0, c.paths, c.dpaths, n_paths=n)
    assert e.value.code == -2
    # nothing to sum: 25 exact zeros
    for over in (dict(n=0), dict(n=-3), dict(E=1), dict(E=0)):
        rc, out = _raw(hip, book, c, "collateralised", **over)
        assert rc == 0 and (out == 0.0).all() and not np.signbit(out).any(), over
    rc, out = _raw(hip, book, c, "collateralised")                              # and the handle serves the next call
    assert rc == 0 and out.tobytes() == ok.tobytes()


def test_census(hip):
    """prints, per record, the row closest to its bound over everything this module ran (it runs last)"""
    assert set(WORST) == set(XT.EVALUATIONS)
    for name in XT.EVALUATIONS:
        frac, y, gap, bound, case = WORST[name]
        print(f"census {name}: yardstick {y:.3e} / device gap {gap:.3e} / bound {bound:.3e}  ({frac:.2f} of its bound; {case})")
