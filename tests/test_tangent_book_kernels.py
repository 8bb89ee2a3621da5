"""The dual book kernels (csrc/kt_book.hip downstream of the paths: kt_eval, kt_lsm_step, kt_lsm_batch, kt_cva, kt_profiles,
kt_pick_find / kt_pick_read) per path and per parameter slot against the long-double restatement of
tests/tangent_book_reference.py, which tests/test_tangent_book_reference.py validates on the host.

Inputs are those of tests/tangent_book_cases.py: books compiled on the CPU oracle (the device book is created from the same plan),
host-made paths and tangents at 1, 255 and 257 paths in tensors with a padded leading dimension (n rounded up to 64, plus 64), NaN
in the pad columns and in every (date, state) row no atom names; outputs pre-filled with NaN.  One larger path count per reducing
kernel lies just past its first grid-stride round (cap 256 + 257 paths; cap = 2 n_cu blocks for mcx_tangent_lsm_step, 64 for
mcx_tangent_profiles, 256 for mcx_tangent_pick).

Per-path bound.  A gap is |device - long-double restatement| relative to the largest |entry| of the row (one image of one netting
set / exposure row / state over the compared paths).  The yardstick of a case is the same gap between the restatement's float64 run
and its long-double run on the case's own inputs, floored at 2^-52 (terms of the row's longest event + 4) — the weighted atoms of a
cash or exercise event (main pass, rolled window or summed events, as the kernel at hand reads them), the n_basis monomials of a
polynomial exposure, the two legs of a Black-Scholes exposure, the three factors of a CVA date's summand; the bound is 4
yardsticks (the device's exp / log / erf differ from numpy's by ulps).  Sums are held to n bound max|t| + n 2^-53 sum|t| over the
restatement's summands t.  Nothing of this is taken from the device.  No path of any case lies within 64 bounds of an option kink or
an exercise tie (asserted from the restatement, here and on the host), so no path is left out of any comparison.

A row whose entries cancel between events (at one path a row is a single entry) is held to its condition number instead: (largest
sum of |event| of the row) / (largest |entry|) x 2^-52 (terms + 4), again from the restatement alone (row_bounds); the CVA's tangents,
which may cancel between the dates, likewise.  The one case that needs it: netting at one path, tangent slot 2 of the floating-rate note, -4.4e-4 where its events contribute 0.48: yardstick
3.84e-14, device gap 2.28e-13 (1.0e-16 absolute: the device is right, the restatement's float64 run rounded favourably), bound
1.46e-12.

Measured on the MI355X (yardstick / device gap / bound of the case closest to its bound; DESIGN.md, "The dual book kernels: what is
pinned"):
  mcx_tangent_eval       1.70e-14 / 2.52e-14 / 6.81e-14   flexis K=3, one path
  mcx_tangent_lsm_step   5.56e-15 / 5.85e-15 / 2.22e-14   (2,1), one path; largest gap 1.97e-14 under 8.19e-14, (4,1) at 257 paths
                         moments: at most 0.47 of their tolerance ((2,3), one path); 9.6e-5 of it at 131,329 paths, (3,4)
  mcx_tangent_cva        1.55e-15 / 3.74e-16 / 6.22e-15   collateralised, 255 paths
  mcx_tangent_profiles   within n 2^-53 sum|t| on exact summands;  mcx_tangent_pick: bit for bit

The last test checks that the module reached every route: the nine kt_lsm_step<K, S>, both outcomes of mcx_tangent_eval on bs_expo,
the three unsecured modes of cva / profiles / pick, and a grid-stride round of lsm_step, profiles and pick."""
import math

import numpy as np
import pytest
import torch

import book_reference as R
import tangent_book_cases as TC
import tangent_book_reference as T
from mcx import _abi
from mcx._native import McxError

pytestmark = pytest.mark.gpu
NP = TC.NP
LD = np.longdouble
EPS53 = 2.0 ** -53
SEEN = set()
WORST = {"eval": 0.0, "lsm_step": 0.0, "cva": 0.0}             # worst device gap per kernel (printed by the census)
MODES, ROWS, H = TC.MODES, TC.ROWS, TC.H


def _nan(hip, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=hip.device)


@pytest.fixture(scope="module")
def dbook(hip, oracle):
    """device books, one per (book, n_basis), created from the oracle-compiled plan"""
    made = {}

    def get(name, K):
        if (name, K) not in made:
            made[name, K] = hip.book_create(TC.book(name, K, oracle).plan)
        return made[name, K]
    yield get
    made.clear()


class _Dev:
    """the inputs of one case on the device, leading dimension ld, NaN in the pad"""

    def __init__(self, hip, x):
        self.n, self.ld = x.n, TC.ld_of(x.n)
        self.paths, self.dpaths = hip.from_numpy(TC.padded(x.paths, self.ld)), hip.from_numpy(TC.padded(x.dpaths, self.ld))
        self.datoms, self.coeffs, self.dcoeffs = hip.from_numpy(x.datoms), hip.from_numpy(x.coeffs), hip.from_numpy(x.dcoeffs)


def _report(what, y, gap, bound):
    print(f"{what}: yardstick {y:.3e}, device gap {gap:.3e}, bound {bound:.3e}")
    assert gap <= bound, (what, y, gap, bound)


def _pad_is_plus_zero(a, n):
    pad = a[..., n:]
    assert (pad == 0.0).all() and not np.signbit(pad).any(), "a pad column is not +0.0"


# ---- mcx_tangent_eval ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TC.SIZES)
@pytest.mark.parametrize("name,K", TC.EVAL_BOOKS, ids=TC.EVAL_IDS)
def test_eval_against_the_restatement(name, K, n, hip, oracle, dbook):
    b, book = TC.book(name, K, oracle), dbook(name, K)
    x = TC.inputs(b, n, oracle)
    y, bound, hi, db = TC.eval_case(b, x)
    assert db.smallest_margin() > T.TIE_FACTOR * bound                          # no path near a kink or a tie
    d = _Dev(hip, x)
    plan = b.plan
    NS, rows = plan.n_netting_sets, max(int(plan.n_expo_rows), 1)
    cfs, expo = _nan(hip, 1 + NP, NS, d.ld), _nan(hip, 1 + NP, NS, rows, d.ld)
    if b.ev_param is not None:                                                  # without the slot table the call is refused
        with pytest.raises(McxError) as e:
            hip.tangent_eval(book, d.datoms, d.coeffs, d.dcoeffs, d.paths, d.dpaths, None, n_paths=n, out=(cfs, expo))
        hip.synchronize()
        assert e.value.code == _abi.E_NOT_FUSABLE and bool(torch.isnan(cfs).all()) and bool(torch.isnan(expo).all())
        SEEN.add(("eval", name, "refused"))
    hip.tangent_eval(book, d.datoms, d.coeffs, d.dcoeffs, d.paths, d.dpaths, b.ev_param, n_paths=n, out=(cfs, expo))
    SEEN.add(("eval", name, "taken"))
    c, e = cfs.cpu().numpy(), expo.cpu().numpy()
    if n == 257 and (plan.products["n_states"] > 1).any():                      # the exposure rows of different states are all taken
        for pr in plan.products[plan.products["n_states"] > 1]:
            taken = [len(np.unique(hi.row_state[q])) for q in range(int(pr["ev_begin"]), int(pr["ev_end"])) if q in hi.row_state]
            assert max(taken) >= 2, (name, K)
    _pad_is_plus_zero(c, n)                                                     # the entry zeroes whole rows
    _pad_is_plus_zero(e, n)
    c, e = c[..., :n], e[..., :n]
    assert not np.isnan(c).any() and not np.isnan(e).any()
    # row by row; a row whose entries cancel between events (one path: a single entry) is held to its condition number instead
    gaps = np.concatenate([T.row_gaps(c, hi.cfs).ravel(), T.row_gaps(e, hi.expo).ravel()])
    bounds = np.concatenate([T.row_bounds(hi.cfs, hi.cfs_mag, y, hi.cfs_terms).ravel(), T.row_bounds(hi.expo, hi.expo_mag, y, hi.expo_terms).ravel()])
    k = int(np.argmax(gaps / bounds))
    print(f"eval {name} K={K} n={n}: {int((bounds > bound).sum())} of {len(bounds)} rows held to their condition number; the row closest to its bound:")
    _report(f"eval {name} K={K} n={n}", y, float(gaps[k]), float(bounds[k]))
    assert (gaps <= bounds).all()
    WORST["eval"] = max(WORST["eval"], float(np.max(gaps[bounds <= bound], initial=0.0)))
    # the decisions: mcx_eval_book on the same paths in record mode (the final state shows in the exposure row taken, above)
    ref = R.evaluate(plan, x.paths, coeffs=x.coeffs)
    bits = hip.new_exercise_bits(len(plan.events), n)
    hip.book_set_exercise_replay(book, 1, bits)
    try:
        pcfs, pexpo = hip.eval_book(book, d.paths[:, :, :n])
    finally:
        hip.book_set_exercise_replay(book, 0, None)
    got_bits = bits.cpu().numpy()
    for q, ex in hi.decisions.items():
        assert np.array_equal((got_bits[q] & 1).astype(bool), ex), (name, K, n, q)
    # the value image is the primal kernel's, each within TOL_SCALAR of the entry's magnitude
    assert (np.abs(c[0] - pcfs.cpu().numpy()[:, :n]) <= R.TOL_SCALAR * np.asarray(ref.cfs_M, dtype=np.float64)).all()
    if plan.n_expo_rows > 0:
        assert (np.abs(e[0] - pexpo.cpu().numpy()[:, :, :n]) <= R.TOL_SCALAR * np.asarray(ref.expo_M, dtype=np.float64)).all()


def test_option_at_its_strike_takes_half_the_tangent(hip):
    """a hand-built plan: one option over the single term 0 + 1 x with weight 1 and numeraire 1; where the path value equals the
    strike exactly the tangent is exactly half of dpaths, one ulp above all of it, one ulp below nothing"""
    from mcx.plan import BookCompiler, BookPlan
    comp = BookCompiler(None, [0.0, 1.0], 3)
    comp.atoms.append((1, 0, 0.0, 1.0, 0.0, 0.0, 0.0))
    comp.atom_src.append(None)
    one = comp.const_atom(1.0)
    comp.add_event(_abi.EV_OPTION, 1, one, 0, comp.add_terms([(1.0, 0)]), -1, 0, strike=100.0, sign=1.0)
    prod = np.zeros(1, dtype=_abi.PRODUCT_DTYPE)
    prod["ev_end"], prod["n_states"] = 1, 1
    plan = BookPlan(comp, prod, 1, 0, 0, True, False, 1)
    book = hip.book_create(plan)
    n, ld = 257, TC.ld_of(257)
    rng = np.random.default_rng(3)
    paths = np.full((2, 1, n), np.nan)
    paths[1, 0] = 100.0 + rng.normal(0.0, 5.0, n)
    tie, above, below = [3, 130, 256], [2, 131, 255], [4, 129, 254]
    paths[1, 0, tie], paths[1, 0, above], paths[1, 0, below] = 100.0, np.nextafter(100.0, np.inf), np.nextafter(100.0, -np.inf)
    dpaths = np.full((NP, 2, 1, n), np.nan)
    dpaths[:, 1, 0] = rng.normal(0.0, 1.0, (NP, n))
    w = np.where(paths[1, 0] > 100.0, 1.0, np.where(paths[1, 0] == 100.0, 0.5, 0.0))
    assert (w[tie] == 0.5).all() and (w[above] == 1.0).all() and (w[below] == 0.0).all()
    cfs, expo = _nan(hip, 1 + NP, 1, ld), _nan(hip, 1 + NP, 1, 1, ld)
    hip.tangent_eval(book, hip.zeros(len(plan.atoms), 5, NP), hip.zeros(1), hip.zeros(1, NP), hip.from_numpy(TC.padded(paths, ld)),
                     hip.from_numpy(TC.padded(dpaths, ld)), n_paths=n, out=(cfs, expo))
    got = cfs.cpu().numpy()[:, 0, :n]
    assert np.array_equal(got[0], np.maximum(paths[1, 0] - 100.0, 0.0))
    assert np.array_equal(got[1:], w * dpaths[:, 1, 0])                          # bits of the input, halved at the tie
    rs = T.DualBook(plan, paths, dpaths, np.zeros((len(plan.atoms), 5, NP)), dtype=np.float64).evaluate(np.zeros(1), np.zeros((1, NP)))
    assert np.array_equal(got, rs.cfs[:, 0])


# ---- mcx_tangent_lsm_step ------------------------------------------------------------------------------------------------------------
def _moment_tolerance(t, n, bound):
    """every summand within `bound` of its row's largest, n of them; any summation order within n 2^-53 of the sum of magnitudes"""
    t = np.abs(np.asarray(t, dtype=np.float64))
    return n * bound * t.max(axis=-1) + n * EPS53 * t.sum(axis=-1)


def _lsm_step_run(K, S, n, hip, oracle, dbook):
    name, pname = TC.LSM_STEP[K, S]
    b, book = TC.book(name, K, oracle), dbook(name, K)
    x = TC.inputs(b, n, oracle)
    d = _Dev(hip, x)
    W, dW = _nan(hip, S, d.ld), _nan(hip, NP, S, d.ld)
    W[:, :n], dW[:, :, :n] = 0.0, 0.0
    for k, step in enumerate(b.lsm_steps(pname)):
        W0, dW0 = W.cpu().numpy()[:, :n], dW.cpu().numpy()[:, :, :n]          # the second step runs on the first's output
        (p_i, r0, r1, num, xa, shift, scale), (Wn, dWn, t), y_w, y_t = TC.lsm_step_ref(b, x, b.product(pname), step, W0, dW0)
        assert r1 > r0
        mom = hip.tangent_lsm_step(book, p_i, r0, r1, num, xa, shift, scale, d.datoms, d.paths, d.dpaths, W, dW, n_paths=n)
        SEEN.add(("lsm_step", K, S))
        gW, gdW = W.cpu().numpy(), dW.cpu().numpy()
        assert np.isnan(gW[:, n:]).all() and np.isnan(gdW[:, :, n:]).all()       # the pad is untouched
        gap = max(T.row_gap(gW[:, :n], Wn), T.row_gap(gdW[:, :, :n], dWn))
        WORST["lsm_step"] = max(WORST["lsm_step"], gap)
        _report(f"lsm_step K={K} S={S} n={n} step {k}", y_w, gap, T.FACTOR * y_w)
        tol = _moment_tolerance(t, n, T.FACTOR * y_t)
        gap = np.abs(mom - np.asarray(t.sum(axis=-1), dtype=np.float64))
        print(f"lsm_step K={K} S={S} n={n} step {k}: summand yardstick {y_t:.3e}, worst moment gap / tolerance {float(np.max(gap / np.where(tol > 0, tol, 1))):.3e}")
        assert mom.shape == tol.shape and (gap <= tol).all()


@pytest.mark.parametrize("n", TC.SIZES)
@pytest.mark.parametrize("K,S", sorted(TC.LSM_STEP))
def test_lsm_step_against_the_restatement(K, S, n, hip, oracle, dbook):
    _lsm_step_run(K, S, n, hip, oracle, dbook)


def test_lsm_step_past_its_first_grid_stride_round(hip, oracle, dbook):
    cap = TC.lsm_step_cap(hip.device_info()["n_cu"])
    n = TC.stride_size(cap)
    assert -(-n // TC.BLOCK) > cap                                              # more blocks of paths than the grid has
    _lsm_step_run(3, 4, n, hip, oracle, dbook)
    SEEN.add(("lsm_step", "stride"))


# ---- mcx_tangent_lsm / mcx_tangent_lsm_batch, the plain instantiation ------------------------------------------------------------------
@pytest.mark.parametrize("n", TC.SIZES)
@pytest.mark.parametrize("name", ["den", "netting"])
def test_lsm_and_batch_plain_instantiation(name, n, hip, oracle, dbook):
    b, book = TC.book(name, 3, oracle), dbook(name, 3)
    x = TC.inputs(b, n, oracle)
    d = _Dev(hip, x)
    plan, K = b.plan, 3
    jobs, _ = b.sc._regression_plan()
    table, want, tols = [], [], []
    with_den = False
    for p_sc, _p, sched, atoms in jobs:
        p_i = p_sc + (b.shift if p_sc > 0 else 0)
        pr = plan.products[p_i]
        assert pr["n_states"] == 1
        n_cf = int(pr["cf_end"] - pr["cf_begin"])
        for entry, (num, xa) in zip(sched, atoms):
            first = int(entry[1])
            shift, scale = TC.centering(plan, xa, x.paths)
            res = {}
            for dt in (np.float64, LD):
                rs = T.DualBook(plan, x.paths, x.dpaths, x.datoms, dtype=dt)
                res[dt] = rs.lsm_step(p_i, first, n_cf, num, xa, shift, scale, np.zeros((1, n)), np.zeros((NP, 1, n)), x.coeffs, terms=True)[2]
            longest = rs.longest(int(pr["cf_begin"]) + first, int(pr["cf_end"]))      # of the events the job sums
            y_t = T.yardstick(res[np.float64], res[LD], longest)
            assert rs.smallest_margin() > T.TIE_FACTOR * T.FACTOR * y_t
            table.append((p_i, first, num, xa, shift, scale))
            want.append(np.asarray(res[LD].sum(axis=-1), dtype=np.float64))
            tols.append(_moment_tolerance(res[LD], n, T.FACTOR * y_t))
            ev = range(int(pr["cf_begin"]) + first, int(pr["cf_end"]))
            with_den = with_den or any(plan.terms["den"][j] >= 0 for q in ev for j in range(plan.events["term_begin"][q], plan.events["term_end"][q]))
    assert len(table) >= 2 and with_den                                         # some job sums terms over their own denominators
    tab = np.array(table, dtype=_abi.TANGENT_LSM_JOB_DTYPE)
    batch = hip.tangent_lsm_batch(book, tab, d.datoms, d.paths, d.dpaths, n_paths=n)
    worst = 0.0
    for j, q in enumerate(table):
        single = hip.tangent_lsm(book, q[0], q[1], q[2], q[3], q[4], q[5], d.datoms, d.paths, d.dpaths, n_paths=n)
        assert single.tobytes() == batch[j].tobytes()
        gap = np.abs(single - want[j])
        worst = max(worst, float(np.max(gap / np.where(tols[j] > 0, tols[j], 1))))
        assert (gap <= tols[j]).all(), (name, n, j)
    print(f"lsm {name} n={n}: {len(table)} jobs, worst moment gap / tolerance {worst:.3e}")
    SEEN.add(("lsm", name))


# ---- mcx_tangent_cva -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TC.SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_cva_against_the_restatement(mode, n, hip, oracle, dbook):
    b, book = TC.book("mixed_cva", 3, oracle), dbook("mixed_cva", 3)
    x = TC.inputs(b, n, oracle)
    d = _Dev(hip, x)
    plan, sc = b.plan, b.sc
    rows = sc.metric_exposure_indices.numpy().astype(np.int32)
    surv, cond = (np.array(a, dtype=np.int32) for a in sc._cva_atoms[0])
    assert (plan.atoms["b"][surv] != 0.0).all() and (plan.atoms["col"][surv] >= 0).any()
    threshold, coll, delayed = TC.metric_mode(mode, rows)
    NS, n_rows = plan.n_netting_sets, int(plan.n_expo_rows)
    cfs, expo = _nan(hip, 1 + NP, NS, d.ld), _nan(hip, 1 + NP, NS, n_rows, d.ld)
    hip.tangent_eval(book, d.datoms, d.coeffs, d.dcoeffs, d.paths, d.dpaths, n_paths=n, out=(cfs, expo))
    e = expo.cpu().numpy()
    # the exposure is the kernel's output with exact edge values planted in the value image: u == 0.0, e == +-h, e just outside the band
    scale_h = H * 8.0                                                           # the planted values are of the exposures' size
    rng = np.random.default_rng([7, n])
    planted = np.zeros(n, dtype=bool)
    edges = [0.0, H, -H, np.nextafter(H, np.inf), np.nextafter(-H, -np.inf), -0.0, scale_h, -scale_h]
    for r in range(n_rows):
        at = rng.permutation(n)[:len(edges)]
        e[0, 0, r, at] = [edges[(k + r) % len(edges)] for k in range(len(at))]
        planted[at] = True
    e[..., n:] = np.nan                                                         # (the entry left +0.0 in the pad)
    expo = hip.from_numpy(e)
    host = e[:, 0, :, :n]
    # The sign tests compare input bits, except in the collateralised mode, where e - thr(d) is rounded first: off the planted paths
    # its operands must be exactly zero or the difference 64 bounds away from zero (a condition on the inputs, like the ties).
    # A date's summand pos surv (1 - cond) has three factors: the floor counts 3 terms; a tangent that cancels between the dates
    # is held to its condition number (row_bounds), as the rows of mcx_tangent_eval are
    res = {}
    for dt in (np.float64, LD):
        rs = T.DualBook(plan, x.paths, x.dpaths, x.datoms, dtype=dt)
        res[dt], mag = T.cva(rs, host, rows, surv, cond, threshold, 0.4, coll, delayed, with_mag=True)
    y = T.yardstick(res[np.float64], res[LD], 3)
    bound = T.FACTOR * y
    if coll:
        for m in range(len(rows) - 1):
            if delayed[m] >= 0:
                a_, c_ = host[0, rows[m]].astype(LD), T.thr(T.Dual(host[0, delayed[m]].astype(LD), host[1:, delayed[m]].astype(LD)), LD(threshold)).v
                free = ~planted & ~((a_ == 0) & (c_ == 0))
                assert (np.abs(a_ - c_)[free] > T.TIE_FACTOR * bound * (np.abs(a_) + np.abs(c_))[free]).all(), (mode, n, m)
    if n >= 255:                                                                # both signs of unsecured exposure on every metric date
        for m in range(len(rows) - 1):
            u = T.unsecured(host, int(rows[m]), threshold, coll, -1 if delayed is None else int(delayed[m])).v
            assert (u > 0).any() and (u < 0).any(), (mode, m)
    out = _nan(hip, 1 + NP, d.ld)
    hip.tangent_cva(book, d.datoms, rows, surv, cond, threshold, 0.4, expo, 0, d.paths, d.dpaths, delayed, coll, n_paths=n, out=out)
    got = out.cpu().numpy()
    assert np.isnan(got[:, n:]).all() and not np.isnan(got[:, :n]).any()         # the pad is untouched
    assert np.abs(res[LD][1:]).max() > 0 or n == 1
    gaps, bounds = T.row_gaps(got[:, :n], res[LD]), T.row_bounds(res[LD], mag, y, 3)
    k = int(np.argmax(gaps / bounds))
    WORST["cva"] = max(WORST["cva"], float(gaps.max()))
    print(f"cva {mode} n={n}: {int((bounds > bound).sum())} of {len(bounds)} rows held to their condition number; the row closest to its bound:")
    _report(f"cva {mode} n={n}", y, float(gaps[k]), float(bounds[k]))
    assert (gaps <= bounds).all()
    SEEN.add(("cva", mode))


# ---- mcx_tangent_profiles ------------------------------------------------------------------------------------------------------------
def _fabricated(hip, n):
    """expo [1+NP][1][4][ld] on the device (NaN in the pad) and its first n columns on the host; tangents are multiples of 2^-8, so
    that the difference of two of them is exact"""
    e = TC.fabricated_expo(n)
    e[1:] = np.round(e[1:] * 256.0) / 256.0
    return hip.from_numpy(TC.padded(e[:, None], TC.ld_of(n))), e


def _profile_sizes():
    return TC.SIZES + [TC.stride_size(TC.CAP_PROFILES)]


@pytest.mark.parametrize("n", _profile_sizes())
@pytest.mark.parametrize("mode", MODES)
def test_profiles_against_the_restatement(mode, n, hip):
    dev, e = _fabricated(hip, n)
    threshold, coll, delayed = TC.metric_mode(mode, ROWS)
    t = T.profiles(e, ROWS, threshold, coll, delayed, dtype=np.float64, terms=True)           # [dates][2][NP][n], exact summands
    if n >= 255:
        assert all((t[m, 0] != 0).any() and (t[m, 1] != 0).any() for m in range(len(ROWS)))  # both signs on every date
    want = np.array([[[math.fsum(t[m, s, q]) for q in range(NP)] for s in range(2)] for m in range(len(ROWS))])
    got = hip.tangent_profiles(ROWS, threshold, dev, 0, delayed, coll, n_paths=n)
    tol = n * EPS53 * np.abs(t).sum(axis=-1)
    gap = np.abs(got - want)
    print(f"profiles {mode} n={n}: worst gap / tolerance {float(np.max(gap / np.where(tol > 0, tol, 1))):.3e}")
    assert got.shape == want.shape and (gap <= tol).all()
    SEEN.add(("profiles", mode))
    if n > TC.CAP_PROFILES * TC.BLOCK:
        SEEN.add(("profiles", "stride"))


# ---- mcx_tangent_pick ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TC.SIZES + [TC.stride_size(TC.CAP_PICK)])
@pytest.mark.parametrize("mode", ["thresholded", "collateralised"])
def test_pick_takes_the_smallest_index(mode, n, hip):
    e = TC.fabricated_expo(n, seed=9)
    threshold, coll, delayed = TC.metric_mode(mode, ROWS)
    # dates 0..4: a target that occurs once; twice in different blocks; twice in different grid-stride rounds; not at all; once
    grid = TC.CAP_PICK * TC.BLOCK
    pairs = {1: (3, 256) if n > 256 else None, 2: (700, grid + 5) if n > grid + 5 else ((1, 200) if n > 200 else None)}
    once = min(n - 1, 77)
    e[0, :, once] = (5.5 + 0.25 * np.arange(e.shape[1])) * H                    # outside the band: the tangent picked is not zero
    for m, pair in pairs.items():
        if pair is not None:                                                    # the later path copies the earlier one's VALUES only
            e[0, :, pair[0]] = (3.0 + m + (0.25 + 0.07 * m) * np.arange(e.shape[1])) * H        # (distinct per date, also as row differences)
            e[0, :, pair[1]] = e[0, :, pair[0]]
    dev = hip.from_numpy(TC.padded(e[:, None], TC.ld_of(n)))
    u = [T.unsecured(e, int(ROWS[m]), threshold, coll, -1 if delayed is None else int(delayed[m]), dtype=np.float64) for m in range(len(ROWS))]
    targets = np.array([u[0].v[once], u[1].v[pairs[1][0]] if pairs[1] else u[1].v[0], u[2].v[pairs[2][0]] if pairs[2] else u[2].v[0],
                        12345.678, u[4].v[n - 1]])
    want = T.pick(e, ROWS, threshold, targets, coll, delayed)
    hits = [int((u[m].v == targets[m]).sum()) for m in range(len(ROWS))]
    assert hits[3] == 0 and hits[0] >= 1 and want[3].tolist() == [-1.0] + [0.0] * NP
    for m, pair in pairs.items():
        if pair is not None:
            assert hits[m] >= 2 and want[m, 0] == pair[0] and not np.array_equal(u[m].d[:, pair[0]], u[m].d[:, pair[1]])
    got = hip.tangent_pick(ROWS, threshold, targets, dev, 0, delayed, coll, n_paths=n)
    assert got.tobytes() == want.tobytes(), (mode, n, got, want)                # index and tangent: bits copied from the input
    SEEN.add(("pick", mode))
    if n > grid:
        SEEN.add(("pick", "stride"))


def test_pick_unthresholded(hip):
    n = 257
    e = TC.fabricated_expo(n, seed=11)
    e[0, :, 200] = e[0, :, 20]
    targets = np.array([e[0, ROWS[0], 20], 0.5, e[0, ROWS[2], 256], e[0, ROWS[3], 0], e[0, ROWS[4], 20]])
    want = T.pick(e, ROWS, 0.0, targets)
    assert want[0, 0] == 20.0 and want[1, 0] == -1.0 and want[4, 0] == 20.0
    got = hip.tangent_pick(ROWS, 0.0, targets, hip.from_numpy(TC.padded(e[:, None], TC.ld_of(n))), 0, n_paths=n)
    assert got.tobytes() == want.tobytes()
    SEEN.add(("pick", "unthresholded"))


# ---- census --------------------------------------------------------------------------------------------------------------------------
def test_every_route_was_reached(hip):
    """reads what the other tests of this module recorded in SEEN: it holds only when the whole module ran in one process (a -k
    selection or a run split over workers leaves routes unreached that the kernels are not to blame for)"""
    want = {("lsm_step", K, S) for K, S in TC.LSM_STEP} | {("lsm_step", "stride"), ("eval", "bs_expo", "refused"), ("eval", "bs_expo", "taken")}
    want |= {(k, m) for k in ("cva", "profiles", "pick") for m in MODES} | {("profiles", "stride"), ("pick", "stride")}
    want |= {("lsm", "den"), ("lsm", "netting")}
    assert len(TC.LSM_STEP) == 9
    assert want <= SEEN, ("routes not reached (was the whole module run, in one process?)", sorted(want - SEEN, key=str))
    print("worst device gap per kernel:", {k: f"{v:.3e}" for k, v in WORST.items()})
