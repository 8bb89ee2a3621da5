"""kt_fva (csrc/kt_book.hip) through the C ABI, mcx_tangent_fva: per path and per parameter slot against the long-double restatement of
tests/fva_tangent_reference.py, which tests/test_fva_tangent_host.py validates on the host.

Inputs are those of tests/xva_tangent_cases.py: the xva_cases book compiled on the CPU oracle at 2 and 11 metric dates (the device
book is created from the same plan), host-made paths, tangents and atom tangents at 1, 255 and 257 paths in tensors with a padded
leading dimension, NaN in the pad and in every (date, state) row no atom names.  The exposures are mcx_tangent_eval's output; every
image of the first row (the swap starts at par: 1e-4 of the other rows and of one sign) is multiplied by +-128 alternating over the
paths, which is exact, and exact edges are planted in the value image of every row: +-0.0, +-h, the neighbours of +-h outside the
band, +-8h.  At 255 and 257 paths the unsecured exposure is positive on at least a quarter of the (date, path) cells and negative on
at least a quarter, in all three unsecured modes (asserted; measured on the CPU restatement: 0.39 to 0.51 each).  The weights are
those of fva_reference's two curves on the case's timeline; the identities also use a table of exact zeros, a negative table and
unit weights.

Per-path bound.  One-path calls on column i of the padded tensors give the per-path records [3][1+NP][n].  A gap is |device -
long-double restatement| relative to the largest |entry| of the row (one image of one record over the paths).  The yardstick of a
record is the same gap between the restatement's float64 run and its long-double run, floored at 2^-52 (4 + 4): four factors per
summand; the bound is 4 yardsticks.  A row that cancels between the dates or between the legs (the tangents, fva, any row at one
path) is held to its condition number instead (tangent_book_reference.row_bounds).  The sums of a full call are held to
n bound max|t| + n 2^-53 sum|t| over the restatement's summands t.  Nothing is taken from the device.

The census this module prints with `pytest -s` (yardstick / device gap / bound of the row closest to its bound) is copied into
README.md, "Forward-mode FVA".  The workspace refusal cannot be reached through the entry point (1024 x 15 partials always fit the
handle's workspace and pinned buffer: a static_assert), so it is not among the refusals tested."""
import ctypes as C

import numpy as np
import pytest
import torch

import fva_tangent_cases as FC
import fva_tangent_reference as FT
import tangent_book_cases as TC
import tangent_book_reference as T
import xva_tangent_cases as XC
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
        e[:, 0, 0, :n] *= 128.0 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)    # both signs on the first date too (exact)
        self.planted = XC.plant(e, n)
        e[..., n:] = np.nan
        self.e = e
        self.expo = hip.from_numpy(e)
        self.host = e[:, 0, :, :n]


def _case(hip, oracle, dbook, E, n):
    if (E, n) not in _CASES:
        _CASES[E, n] = _Case(hip, oracle, dbook(E), E, n)
    return _CASES[E, n]


def _call(hip, book, c, mode, which, lo=0, hi=None, kind="curves", expo=None, datoms=None, dpaths=None, swap_names=False,
          swap_weights=False, out=None):
    """mcx_tangent_fva on the paths [lo, hi) of the case, as path slices of the padded tensors"""
    hi = c.n if hi is None else hi
    threshold, coll, delayed = XC.metric_mode(mode, c.b.rows)
    cp, own = FC.names(c.b, which)
    wb, wl = FC.weights(c.b.E, kind)
    if swap_names:
        cp, own = own, cp
    if swap_weights:
        wb, wl = wl, wb
    expo = c.expo if expo is None else expo
    dpaths = c.dpaths if dpaths is None else dpaths
    return hip.tangent_fva(book, c.datoms if datoms is None else datoms, c.b.rows, cp, own, wb, wl, threshold, expo[..., lo:hi], 0,
                           c.paths[:, :, lo:hi], dpaths[..., lo:hi], delayed, coll, out=out)


def _per_path(hip, book, c, mode, which, **kw):
    return np.stack([_call(hip, book, c, mode, which, i, i + 1, **kw) for i in range(c.n)], axis=-1)          # [3][1+NP][n]


def _note(r, y, gap, bound, case):
    name = FT.EVALUATIONS[r]
    if name not in WORST or gap / bound > WORST[name][0]:
        WORST[name] = (gap / bound, y, gap, bound, case)


def _sum_tol(hi, rb):
    """of the sums [3][1+NP] over the n paths, every row at its own per-path bound"""
    return np.stack([FT.sum_tolerance(hi[r], rb[r]) for r in range(3)])


@pytest.mark.parametrize("which", FC.SIDES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("E", FC.DATES)
@pytest.mark.parametrize("n", TC.SIZES)
def test_fva_against_the_restatement(n, E, mode, which, hip, oracle, dbook):
    book, c = dbook(E), _case(hip, oracle, dbook, E, n)
    b = c.b
    threshold, coll, delayed = XC.metric_mode(mode, b.rows)
    res, mag = FC.restated(b, c.x, c.host, mode, which)
    y, rb = FC.bounds(res, mag)
    hi = res[LD]
    if coll:        # e - thr(d) is rounded before its sign is read: off the planted paths the difference is exactly 0 or far from 0
        for m in range(E - 1):
            if delayed[m] >= 0:
                a_ = c.host[0, b.rows[m]].astype(LD)
                c_ = T.thr(T.Dual(c.host[0, delayed[m]].astype(LD), c.host[1:, delayed[m]].astype(LD)), LD(threshold)).v
                free = ~c.planted & ~((a_ == 0) & (c_ == 0))
                assert (np.abs(a_ - c_)[free] > T.TIE_FACTOR * 4.0 * y.max() * (np.abs(a_) + np.abs(c_))[free]).all(), (mode, n, m)
    if n >= 255:                   # a condition on the inputs: both signs of unsecured exposure on a quarter of the cells each
        u = FC.unsecured_images(b, c.host, mode)[:, 0]
        assert (u > 0).mean() >= 0.25 and (u < 0).mean() >= 0.25, (mode, n, (u > 0).mean(), (u < 0).mean())
    got = _per_path(hip, book, c, mode, which)                                 # one-path calls on column i
    assert not np.isnan(got).any()
    case = f"n={n} E={E} {mode} {which}"
    for r in range(3):
        gaps = T.row_gaps(got[r], hi[r])
        k = int(np.argmax(gaps / rb[r]))
        print(f"fva {FT.EVALUATIONS[r]} {case}: yardstick {y[r]:.3e}, device gap {gaps[k]:.3e}, bound {rb[r][k]:.3e}"
              f" ({int((rb[r] > 4.0 * y[r]).sum())} of {1 + NP} rows held to their condition number)")
        _note(r, y[r], float(gaps[k]), float(rb[r][k]), case)
        assert (gaps <= rb[r]).all(), (case, FT.EVALUATIONS[r], gaps, rb[r])
    if n > 1:
        assert np.abs(hi[2, 1:]).max() > 0 and np.abs(hi[:, 0]).max() > 0
    # the sums of the full call
    sums = _call(hip, book, c, mode, which)
    tol = _sum_tol(hi, rb)
    want = hi.sum(axis=-1)
    gap = np.abs(sums.astype(LD) - want).astype(np.float64)
    print(f"fva sums {case}: worst gap / tolerance {float(np.max(gap / np.where(tol > 0, tol, 1))):.3e}")
    assert (gap <= tol).all(), (case, gap, tol)
    # the value sums over the paths, divided by n, are the means of mcx_reduce_fva on the same names and weights, at the sum bound
    cp, own = FC.names(b, which)
    wb, wl = FC.weights(E)
    spec = UnsecuredSpec(b.rows, delayed, threshold, coll)
    rec = hip.reduce_fva(book, spec, cp, own, wb, wl, c.expo[0, 0][:, :n], c.paths[:, :, :n])
    mean = rec["shift"] + rec["s1"] / rec["n"]
    mgap, mtol = np.abs(sums[:, 0] / n - mean), tol[:, 0] / n
    print(f"fva means {case}: worst |sum / n - mcx_reduce_fva mean| / tolerance {float(np.max(mgap / np.where(mtol > 0, mtol, 1))):.3e}")
    assert (mgap <= mtol).all(), (case, sums[:, 0] / n, mean, mtol)


@pytest.mark.parametrize("mode", MODES)
def test_a_negative_weight_table_against_the_restatement(mode, hip, oracle, dbook):
    """negative borrowing weights (a finite value is taken as it is): fca and its images change sign, per path at the bound"""
    n, E = 255, 11
    book, c = dbook(E), _case(hip, oracle, dbook, E, n)
    res, mag = FC.restated(c.b, c.x, c.host, mode, "both", kind="negative")
    y, rb = FC.bounds(res, mag)
    got = _per_path(hip, book, c, mode, "both", kind="negative")
    assert (got[0, 0] <= 0).all() and (got[0, 0] < 0).any() and (got[1, 0] >= 0).all()
    for r in range(3):
        gaps = T.row_gaps(got[r], res[LD][r])
        assert (gaps <= rb[r]).all(), (mode, FT.EVALUATIONS[r], gaps, rb[r])
        k = int(np.argmax(gaps / rb[r]))
        _note(r, y[r], float(gaps[k]), float(rb[r][k]), f"n={n} E={E} {mode} both, negative borrowing weights")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("E", FC.DATES)
def test_without_names_and_with_unit_weights(E, mode, hip, oracle, dbook):
    """every product is exact then.  Per path, bit for bit and image by image: fca is the sequential float64 sum over the dates of
    the exposure images where x.v > 0, fba that of their negatives where x.v < 0.  And the tangent sums of the full call are the
    sums over the summand dates of mcx_tangent_profiles (another kernel, another reduction), at the sum tolerance"""
    n = 257
    book, c = dbook(E), _case(hip, oracle, dbook, E, n)
    threshold, coll, delayed = XC.metric_mode(mode, c.b.rows)
    got = _per_path(hip, book, c, mode, "none", kind="unit")
    fca, fba = FC.sequential_legs(FC.unsecured_images(c.b, c.host, mode))
    assert np.abs(fca).max() > 0 and np.abs(fba).max() > 0
    assert np.array_equal(got[0], fca) and np.array_equal(got[1], fba) and np.array_equal(got[2], fca - fba)
    sums = _call(hip, book, c, mode, "none", kind="unit")
    res, mag = FC.restated(c.b, c.x, c.host, mode, "none", kind="unit")
    _y, rb = FC.bounds(res, mag)
    tol = _sum_tol(res[LD], rb)
    prof = hip.tangent_profiles(c.b.rows, threshold, c.expo, 0, delayed, coll, n_paths=n)          # [E][2][NP] sums of 1[u>0] du, 1[u<0] du
    want_ca, want_ba = prof[:E - 1, 0].sum(axis=0), -prof[:E - 1, 1].sum(axis=0)
    g = max(float(np.max(np.abs(sums[0, 1:] - want_ca) / tol[0, 1:])), float(np.max(np.abs(sums[1, 1:] - want_ba) / tol[1, 1:])))
    print(f"fva E={E} {mode}: unit weights, no names: tangent sums against mcx_tangent_profiles, worst gap / tolerance {g:.3e}")
    assert g <= 1.0


def test_past_the_first_grid_stride_round(hip, oracle, dbook):
    """cap x 256 + 257 paths at 2 metric dates: the second round of the grid stride adds into the lanes' sums"""
    n = TC.stride_size(FC.GRID_CAP)
    book, c = dbook(2), _Case(hip, oracle, dbook(2), 2, n)
    mode, which = "thresholded", "both"
    res, mag = FC.restated(c.b, c.x, c.host, mode, which)
    _y, rb = FC.bounds(res, mag)
    tol = _sum_tol(res[LD], rb)
    sums = _call(hip, book, c, mode, which)
    half = n // 2
    halves = _call(hip, book, c, mode, which, 0, half) + _call(hip, book, c, mode, which, half, n)
    want = res[LD].sum(axis=-1)
    g1, g2 = np.abs(sums.astype(LD) - want).astype(np.float64), np.abs(sums - halves)
    print(f"fva grid stride n={n}: worst gap / tolerance {float(np.max(g1 / tol)):.3e} (restatement), {float(np.max(g2 / tol)):.3e} (halves)")
    assert (np.abs(sums) > 0).all() and (g1 <= tol).all() and (g2 <= tol).all()
    assert sums.tobytes() == _call(hip, book, c, mode, which).tobytes()


@pytest.mark.parametrize("mode", ["unthresholded", "collateralised"])
def test_device_identities(mode, hip, oracle, dbook):
    n, E = 257, 11
    book, c = dbook(E), _case(hip, oracle, dbook, E, n)
    both = _call(hip, book, c, mode, "both")
    assert both.tobytes() == _call(hip, book, c, mode, "both").tobytes()                 # two calls: identical bytes
    assert (both[:2, 0] > 0).all() and np.abs(both[:, 1:]).min() > 0
    # the weight tables swapped and every exposure image negated: the legs change places, fva changes sign, bit for bit in every image
    neg = hip.from_numpy(-c.e)
    sw = _call(hip, book, c, mode, "both", expo=neg, swap_weights=True)
    assert sw[0].tobytes() == both[1].tobytes() and sw[1].tobytes() == both[0].tobytes() and sw[2].tobytes() == (-both[2]).tobytes()
    # the names swapped: w.v = S_c.v S_o.v commutes, so the value images keep their bytes; the tangent of w adds the same two
    # products with the other one inside the fused multiply-add, so the tangent images move by roundings: per path at the bound
    pp = _per_path(hip, book, c, mode, "both")
    ps = _per_path(hip, book, c, mode, "both", swap_names=True)
    assert ps[:, 0].tobytes() == pp[:, 0].tobytes()
    res, mag = FC.restated(c.b, c.x, c.host, mode, "both")
    _y, rb = FC.bounds(res, mag)
    gaps = np.stack([T.row_gaps(ps[r], pp[r]) for r in range(3)])
    print(f"fva {mode}: names swapped, tangent images: worst gap {gaps[:, 1:].max():.3e} (worst gap / bound {(gaps / rb)[:, 1:].max():.3e})")
    assert (gaps <= rb).all()
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
    # zero lending weights: fba is zero and fva is fca in every image; fca keeps its bytes
    zl = _call(hip, book, c, mode, "both", kind="zero_lend")
    assert (zl[1] == 0.0).all() and zl[2].tobytes() == zl[0].tobytes() and zl[0].tobytes() == both[0].tobytes()
    # a name that never defaults is the constant 1: with neither, unit weights and this call's names, all four choices give finite sums
    for which in FC.SIDES:
        s = _call(hip, book, c, mode, which)
        assert np.isfinite(s).all() and (s[:2, 0] > 0).all()


def _raw(hip, book, c, mode, **over):
    """the entry point itself with one argument replaced -> (status, the poisoned output)"""
    threshold, coll, delayed = XC.metric_mode(mode, c.b.rows)
    out = np.full((3, 1 + NP), 777.0)
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
    wb, wl = FC.weights(c.b.E)
    a = dict(rows=i32(c.b.rows), delayed=i32(delayed), sc=i32(c.b.cp[0]), so=i32(c.b.own[0]), wb=wb, wl=wl, n=c.n, ld=c.ld, E=len(c.b.rows),
             out=out, handle=hip.h, book_ptr=book.ptr, expo=c.expo[0, 0], paths=c.paths, dpaths=c.dpaths, datoms=c.datoms)
    a.update(over)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = hip.lib.mcx_tangent_fva(a["handle"], a["book_ptr"], vp(a["datoms"]), _abi.ptr(a["rows"]), _abi.ptr(a["delayed"]), C.c_int32(int(coll)),
                                 C.c_int32(a["E"]), C.c_double(threshold), _abi.ptr(a["sc"]), _abi.ptr(a["so"]), _abi.ptr(a["wb"]),
                                 _abi.ptr(a["wl"]), vp(a["expo"]), C.c_int64(c.expo.stride(0)), vp(a["paths"]), vp(a["dpaths"]),
                                 C.c_int64(a["n"]), C.c_int64(a["ld"]), C.c_int32(c.paths.shape[0]), _abi.ptr(a["out"]), hip._stream())
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
        ("atom out of range", dict(sc=bad(b.cp[0], 3, n_atoms))), ("atom out of range", dict(sc=bad(b.cp[0], 0, -1))),
        ("atom out of range", dict(so=bad(b.own[0], E - 2, n_atoms))), ("atom out of range", dict(so=bad(b.own[0], 1, n_atoms + 5))),
        ("exposure row", dict(rows=bad(b.rows, 2, n_rows))), ("exposure row", dict(rows=bad(b.rows, E - 1, -1))),
        ("exposure row", dict(delayed=bad(delayed, 4, n_rows))),
        ("leading dimension", dict(ld=n - 1)),
    ]
    for text, over in refusals:
        rc, out = _raw(hip, book, c, "collateralised", **over)
        assert rc == -2 and (out == 777.0).all(), (text, over, rc)
        assert text in hip.lib.mcx_last_error(hip.h).decode(), (text, hip.lib.mcx_last_error(hip.h))
    for over in (dict(book_ptr=None), dict(rows=None), dict(wb=None), dict(wl=None), dict(out=None), dict(datoms=None), dict(expo=None),
                 dict(paths=None), dict(dpaths=None)):
        rc, out = _raw(hip, book, c, "collateralised", **over)
        assert rc == -1 and (out == 777.0).all(), over
        assert "NULL" in hip.lib.mcx_last_error(hip.h).decode(), over
    rc, out = _raw(hip, book, c, "collateralised", handle=None)                 # (no handle to carry a message)
    assert rc == -1 and (out == 777.0).all()
    with pytest.raises(McxError) as e:                                          # the binding raises what the library refuses
        hip.tangent_fva(book, c.datoms, bad(b.rows, 0, n_rows), b.cp[0], b.own[0], *FC.weights(E), 0.0, c.expo, 0, c.paths, c.dpaths, n_paths=n)
    assert e.value.code == -2
    # nothing to sum: 15 exact zeros
    for over in (dict(n=0), dict(n=-3), dict(E=1), dict(E=0)):
        rc, out = _raw(hip, book, c, "collateralised", **over)
        assert rc == 0 and (out == 0.0).all() and not np.signbit(out).any(), over
    rows1 = hip.tangent_fva(book, c.datoms, b.rows[:1], None, None, np.zeros(0), np.zeros(0), 0.0, c.expo, 0, c.paths, c.dpaths, n_paths=n)
    assert rows1.shape == (3, 1 + NP) and (rows1 == 0.0).all()                  # one metric date through the binding
    rc, out = _raw(hip, book, c, "collateralised")                              # and the handle serves the next call
    assert rc == 0 and out.tobytes() == ok.tobytes()


def test_census(hip):
    """prints, per record, the row closest to its bound over everything this module ran (it runs last)"""
    assert set(WORST) == set(FT.EVALUATIONS)
    for name in FT.EVALUATIONS:
        frac, y, gap, bound, case = WORST[name]
        print(f"census {name}: yardstick {y:.3e} / device gap {gap:.3e} / bound {bound:.3e}  ({frac:.2f} of its bound; {case})")
