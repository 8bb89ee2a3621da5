"""The restatement of the dual book program (tests/tangent_book_reference.py) validated on the host, before the GPU tests trust it:

  (a) in long double its value image is book_reference.evaluate on the same plan, paths and coefficients, to 1e-17 of the entry's
      magnitude M: cashflows, exposures, every exercise decision and final state;
  (b) its tangents are the central differences of book_reference.evaluate in long double along the direction (datoms, dpaths,
      dcoeffs; sigma and rate of a Black-Scholes exposure in their slots), exercise decisions frozen through `replay`, at the step
      2^-20 (0.95e-6; a power of two keeps x +- h dx exact in float64, see tangent_book_cases).  Agreement is to the truncation
      term: |tangent - FD(h/2)| <= |FD(h) - FD(h/2)| (three times FD(h/2)'s own truncation error) plus the long-double rounding of
      the differenced values, 32 2^-64 M / h.  Each case prints the largest truncation term it met, relative to its row;
  (c) the same for lsm_step, two consecutive steps per (K, S), on 64 paths: the roll is restated through book_reference.evaluate on
      a one-product plan that starts in each hypothetical state (controller.py:316-383: cashflows of the window along the policy
      plus the cached tail of the state the roll ends in), the moment sums through lsm_reference.moments_ref;
  (d) the conditions on the inputs of tests/tangent_book_cases.py: no path within 64 bounds of an option kink or an exercise tie,
      every exercise state populated at 257 paths;
  (e) the exact edges of unsecured / cva / profiles / pick on hand-made exposures: h, -h, nextafter(h, inf), 0.0, -0.0, NaN."""
import copy

import numpy as np
import pytest

import book_reference as R
import lsm_reference
import tangent_book_cases as TC
import tangent_book_reference as T
from mcx import _abi
from payoff_tangent_reference import Dual

LD = np.longdouble
NP = TC.NP
H = 2.0 ** -20
EV_IDS = TC.EVAL_IDS


def _run(b, x, dtype=LD):
    db = T.DualBook(b.plan, x.paths, x.dpaths, x.datoms, dtype=dtype)
    return db, db.evaluate(x.coeffs, x.dcoeffs, b.ev_param)


def _within(got, ref, M, tol):
    err = np.abs(got - ref)
    assert (err <= tol * M).all(), float(np.max(err / np.where(M > 0, M, 1)))


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TC.SIZES)
@pytest.mark.parametrize("name,K", TC.EVAL_BOOKS, ids=EV_IDS)
def test_value_image_is_the_primal_interpreter(name, K, n, oracle):
    b = TC.book(name, K, oracle)
    x = TC.inputs(b, n, oracle)
    _db, run = _run(b, x)
    ref = R.evaluate(b.plan, x.paths, coeffs=x.coeffs)
    _within(run.cfs[0], ref.cfs, ref.cfs_M, LD(1e-17))
    _within(run.expo[0], ref.expo, ref.expo_M, LD(1e-17))
    assert set(run.decisions) == set(ref.decisions)
    for q in ref.decisions:
        assert np.array_equal(run.decisions[q], ref.decisions[q]), q
    assert np.array_equal(run.final_state, ref.final_state)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
def _moved(b, x, q, h):
    """(plan, paths, coeffs) moved by h along direction q; every moved number is exact"""
    plan = copy.copy(b.plan)
    plan.atoms = b.plan.atoms.copy()
    for j, f in enumerate(("a", "d", "b", "c0", "c1")):
        plan.atoms[f] = b.plan.atoms[f] + h * x.datoms[:, j, q]
        assert ((plan.atoms[f].astype(LD) - b.plan.atoms[f].astype(LD)) == LD(h) * x.datoms[:, j, q].astype(LD)).all(), f
    paths = x.paths + h * x.dpaths[q]
    ok = ~np.isnan(x.paths)
    assert ((paths[ok].astype(LD) - x.paths[ok].astype(LD)) == LD(h) * x.dpaths[q][ok].astype(LD)).all()
    coeffs = x.coeffs + h * x.dcoeffs[:, q]
    assert ((coeffs.astype(LD) - x.coeffs.astype(LD)) == LD(h) * x.dcoeffs[:, q].astype(LD)).all()
    if b.ev_param is not None:
        plan.events = b.plan.events.copy()
        for k in (0, 1):
            sel = b.ev_param[:, k] == q
            plan.events["aux"][sel, k] += h
            assert ((plan.events["aux"][sel, k].astype(LD) - b.plan.events["aux"][sel, k].astype(LD)) == LD(h)).all()
    return plan, paths, coeffs


def _fd(b, x, q, h, replay):
    (pu, xu, cu), (pd, xd, cd) = _moved(b, x, q, h), _moved(b, x, q, -h)
    up, dn = R.evaluate(pu, xu, replay=replay, coeffs=cu), R.evaluate(pd, xd, replay=replay, coeffs=cd)
    return (up.cfs - dn.cfs) / LD(2 * h), (up.expo - dn.expo) / LD(2 * h)


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("name,K", TC.EVAL_BOOKS, ids=EV_IDS)
def test_tangents_are_central_differences_of_the_primal_interpreter(name, K, n, oracle):
    b = TC.book(name, K, oracle)
    x = TC.inputs(b, n, oracle)
    _db, run = _run(b, x)
    ref = R.evaluate(b.plan, x.paths, coeffs=x.coeffs)
    replay = {q: ref.decisions.get(q, np.zeros(n, dtype=bool)) for q in range(len(b.plan.events))}
    worst = 0.0
    for q in range(NP):
        coarse, fine = _fd(b, x, q, H, replay), _fd(b, x, q, H / 2, replay)
        for got, c, f, M in ((run.cfs[1 + q], coarse[0], fine[0], ref.cfs_M), (run.expo[1 + q], coarse[1], fine[1], ref.expo_M)):
            trunc = np.abs(c - f)
            assert (np.abs(got - f) <= trunc + 32 * LD(2.0) ** -64 * M / LD(H)).all(), (name, K, n, q)
            scale = np.abs(got).max(axis=-1, keepdims=True)
            worst = max(worst, float(np.max(trunc / np.where(scale > 0, scale, 1))))
    assert np.abs(run.cfs[1:]).max() > 0 and np.abs(run.expo[1:]).max() > 0
    print(f"{name} K={K} n={n}: largest truncation term |FD(h) - FD(h/2)| / row's largest tangent = {worst:.3e}")


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def _roll_ref(plan, pr, q0, q1, S, paths, coeffs, W, replay=None):
    """W' [S][n] and the decisions {s0: {event: bits}}: the window [q0, q1) through book_reference.evaluate from every start state"""
    one = copy.copy(plan)
    out, bits, mags = [], {}, []
    cols = np.arange(paths.shape[2])
    for s0 in range(S):
        row = np.zeros(1, dtype=_abi.PRODUCT_DTYPE)
        row["ev_begin"], row["ev_end"], row["init_state"], row["n_states"] = q0, q1, s0, S
        one.products = row
        r = R.evaluate(one, paths, coeffs=coeffs, replay=None if replay is None else replay[s0])
        bits[s0] = {q: r.decisions.get(q, np.zeros(len(cols), dtype=bool)) for q in range(len(plan.events))}
        tail = np.asarray(W, dtype=LD)[r.final_state[0], cols]
        out.append(r.cfs[0] + tail)
        mags.append(r.cfs_M[0] + np.abs(tail))
    return np.stack(out), bits, np.stack(mags)


def _summands_ref(plan, K, S, num_atom, x_atom, shift, scale, paths, Wn):
    num, z = R.atom(plan, num_atom, paths)[0], (R.atom(plan, x_atom, paths)[0] - LD(shift)) * LD(scale)
    t = [z ** k for k in range(2 * K - 1)]
    return np.stack(t + [z ** k * (num * Wn[s]) for s in range(S) for k in range(K)]), z, num


@pytest.mark.parametrize("K,S", sorted(TC.LSM_STEP))
def test_lsm_step_against_a_direct_restatement(K, S, oracle):
    name, pname = TC.LSM_STEP[K, S]
    b = TC.book(name, K, oracle)
    n = 64
    x = TC.inputs(b, n, oracle)
    plan = b.plan
    p_i = b.product(pname)
    pr = plan.products[p_i]
    assert int(pr["n_states"]) == S
    W, dW = np.zeros((S, n)), np.zeros((NP, S, n))
    for step, (r0, r1, num_atom, x_atom) in enumerate(b.lsm_steps(pname)):
        shift, scale = TC.centering(plan, x_atom, x.paths)
        db = T.DualBook(plan, x.paths, x.dpaths, x.datoms)
        Wn, dWn, t = db.lsm_step(p_i, r0, r1, num_atom, x_atom, shift, scale, W, dW, x.coeffs, terms=True)
        q0, q1 = int(pr["cf_begin"]) + r0, int(pr["cf_begin"]) + r1
        Wref, bits, WM = _roll_ref(plan, pr, q0, q1, S, x.paths, x.coeffs, W)
        tref, z, num = _summands_ref(plan, K, S, num_atom, x_atom, shift, scale, x.paths, Wref)
        # magnitudes: z = (x - shift) scale cancels, so its rounding is that of (mag(x) + |shift|) scale, not of |z|
        zM = (R.atom(plan, x_atom, x.paths)[1] + abs(LD(shift))) * LD(scale)
        tM = np.stack([zM ** k if k else np.zeros(n, dtype=LD) for k in range(2 * K - 1)] + [zM ** k * np.abs(num) * WM[s] for s in range(S) for k in range(K)])
        assert (np.abs(Wn - Wref) <= LD(1e-17) * WM).all()
        assert (np.abs(t[0] - tref) <= LD(1e-17) * tM).all()
        m_ref, mag = lsm_reference.moments_ref(np.asarray(z, dtype=np.float64), np.asarray(num * Wref, dtype=np.float64), K)
        assert (np.abs(np.asarray(t[0].sum(axis=-1), dtype=np.float64) - m_ref) <= 8 * 2.0 ** -53 * (2 * K) * mag).all()
        worst = 0.0
        for q in range(NP):
            fd = {}
            for h in (H, H / 2):
                side = []
                for sgn in (1.0, -1.0):
                    pl, pa, co = _moved(b, x, q, sgn * h)
                    Wm = W + sgn * h * dW[q]
                    assert ((Wm.astype(LD) - W.astype(LD)) == LD(sgn * h) * dW[q].astype(LD)).all()
                    Wr, _, _ = _roll_ref(pl, pr, q0, q1, S, pa, co, Wm, replay=bits)
                    side.append((Wr, _summands_ref(pl, K, S, num_atom, x_atom, shift, scale, pa, Wr)[0]))
                fd[h] = ((side[0][0] - side[1][0]) / LD(2 * h), (side[0][1] - side[1][1]) / LD(2 * h))
            for got, c, f, M in ((dWn[q], fd[H][0], fd[H / 2][0], WM), (t[1 + q], fd[H][1], fd[H / 2][1], tM)):
                trunc = np.abs(c - f)
                assert (np.abs(got - f) <= trunc + 32 * LD(2.0) ** -64 * M / LD(H)).all(), (K, S, step, q)
                scale_ = np.abs(got).max(axis=-1, keepdims=True)
                worst = max(worst, float(np.max(trunc / np.where(scale_ > 0, scale_, 1))))
        assert np.abs(dWn).max() > 0
        print(f"lsm_step K={K} S={S} step {step}: window [{r0}, {r1}), largest truncation term / row's largest tangent = {worst:.3e}")
        W, dW = np.asarray(Wn, dtype=np.float64), TC.quantize(np.asarray(dWn, dtype=np.float64), np.asarray(Wn, dtype=np.float64)[None])


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TC.SIZES)
@pytest.mark.parametrize("name,K", TC.EVAL_BOOKS, ids=EV_IDS)
def test_no_path_is_near_a_kink_or_a_tie(name, K, n, oracle):
    b = TC.book(name, K, oracle)
    x = TC.inputs(b, n, oracle)
    y, bound, hi, db = TC.eval_case(b, x)
    print(f"{name} K={K} n={n}: yardstick {y:.3e}, smallest margin {db.smallest_margin():.3e} (must exceed {T.TIE_FACTOR * bound:.3e})")
    assert db.smallest_margin() > T.TIE_FACTOR * bound
    if n == 257:
        for p_i, pr in enumerate(b.plan.products):
            if pr["n_states"] > 1:
                assert (np.bincount(hi.final_state[p_i], minlength=int(pr["n_states"])) >= 1).all(), (name, K, p_i, np.bincount(hi.final_state[p_i]))


@pytest.mark.parametrize("K,S", sorted(TC.LSM_STEP))
def test_no_lsm_step_path_is_near_a_kink_or_a_tie(K, S, oracle):
    name, pname = TC.LSM_STEP[K, S]
    b = TC.book(name, K, oracle)
    for n in TC.SIZES + ([TC.stride_size(TC.lsm_step_cap(TC.N_CU_MI355X))] if (K, S) == (3, 4) else []):
        x = TC.inputs(b, n, oracle)
        W, dW = np.zeros((S, n)), np.zeros((NP, S, n))
        for step in b.lsm_steps(pname):
            _args, (Wn, dWn, _t), _y_w, _y_t = TC.lsm_step_ref(b, x, b.product(pname), step, W, dW)
            W, dW = np.asarray(Wn, dtype=np.float64), np.asarray(dWn, dtype=np.float64)


@pytest.mark.parametrize("mode", TC.MODES)
def test_both_signs_of_unsecured_exposure_on_every_metric_date(mode):
    """the fabricated exposures of the profile and pick tests, at every size but the single path"""
    threshold, coll, delayed = TC.metric_mode(mode, TC.ROWS)
    for n in TC.SIZES[1:] + [TC.stride_size(TC.CAP_PROFILES), TC.stride_size(TC.CAP_PICK)]:
        e = TC.fabricated_expo(n)
        for m in range(len(TC.ROWS)):
            u = T.unsecured(e, int(TC.ROWS[m]), threshold, coll, -1 if delayed is None else int(delayed[m]), dtype=np.float64).v
            assert (u > 0).any() and (u < 0).any(), (mode, n, m)


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
THR = TC.H
UP, NAN = np.nextafter(THR, np.inf), float("nan")


def _expo(values, delayed_values=None):
    """[1+NP][2][n]: row 0 = values, row 1 = the delayed row; tangent q of path i is 10 (q + 1) + i (row 1: negative)"""
    n = len(values)
    e = np.zeros((1 + NP, 2, n))
    e[0, 0] = values
    e[0, 1] = values if delayed_values is None else delayed_values
    for q in range(NP):
        e[1 + q, 0] = 10.0 * (q + 1) + np.arange(n)
        e[1 + q, 1] = -(100.0 * (q + 1) + np.arange(n))
    return e


EDGE_VALUES = [THR, -THR, UP, -UP, 0.0, -0.0, NAN, 2 * THR, -2 * THR]


def test_unsecured_at_the_exact_edges():
    e = _expo(EDGE_VALUES)
    u = T.unsecured(e, 0, THR, dtype=np.float64)
    assert np.array_equal(u.v, [0.0, 0.0, UP - THR, -(UP - THR), 0.0, 0.0, 0.0, THR, -THR])          # closed band: value zero (NaN: zero too)
    passes = np.array([0, 0, 1, 1, 0, 0, 0, 1, 1], dtype=bool)
    assert np.array_equal(u.d, np.where(passes, e[1:, 0], 0.0))                                # ... and tangent zero
    u0 = T.unsecured(e, 0, 0.0, dtype=np.float64)                                              # THR == 0: nothing is thresholded
    assert np.array_equal(u0.v, e[0, 0], equal_nan=True) and np.array_equal(u0.d, e[1:, 0])
    c = T.unsecured(e, 0, THR, True, -1, dtype=np.float64)                                       # collateralised, no delayed row yet
    assert np.array_equal(c.v, e[0, 0], equal_nan=True) and np.array_equal(c.d, e[1:, 0])
    c = T.unsecured(e, 0, THR, True, 1, dtype=np.float64)                                        # E[row] - thr(E[delayed])
    assert np.array_equal(c.v[:6], [THR, -THR, THR, -THR, 0.0, 0.0]) and np.isnan(c.v[6]) and np.array_equal(c.v[7:], [THR, -THR])
    assert np.array_equal(c.d, e[1:, 0] - np.where(passes, e[1:, 1], 0.0))
    c = T.unsecured(e, 0, THR, True, 0, dtype=np.float64)                                        # the delayed row is the row itself
    assert np.array_equal(c.v[[2, 3, 7, 8]], [THR, -THR, THR, -THR])


class _Flat:
    """two atoms that are the same on every path: survival 0.9 and conditional survival 0.8, with tangents"""
    dtype = LD

    def __init__(self, n):
        self.n, self.NP = n, NP

    def uniform(self, c, dc=None):
        return Dual.uniform(LD(c), np.zeros(NP) if dc is None else dc, self.n, LD)

    def atom(self, k):
        return self.uniform(0.9, [0.5, 0.0, 0.0, 0.0]) if k == 0 else self.uniform(0.8, [0.0, 0.25, 0.0, 0.0])


def test_cva_profiles_and_pick_at_the_exact_edges():
    e = _expo(EDGE_VALUES)
    n = len(EDGE_VALUES)
    rows, atoms = [0, 0, 0], ([0, 0], [1, 1])                                                  # three metric dates: two summands
    got = T.cva(_Flat(n), e, rows, atoms[0], atoms[1], THR, 0.4)
    pays = np.array([0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=bool)                                   # strictly positive unsecured exposure only
    u = np.where(pays, np.array(EDGE_VALUES) - THR, 0.0)
    assert np.allclose(np.asarray(got[0], dtype=np.float64), 2 * u * 0.9 * 0.2 * 0.6, rtol=1e-15, atol=0.0)
    assert (got[1:, ~pays] == 0).all() and (got[3, pays] != 0).all()
    want1 = 2 * 0.6 * (e[1, 0] * 0.9 * 0.2 + u * 0.5 * 0.2)                                    # slot 0: exposure and survival tangents
    assert np.allclose(np.asarray(got[1], dtype=np.float64)[pays], want1[pays], rtol=1e-15)
    p = T.profiles(e, [0, 1], THR, dtype=np.float64)
    pos, neg = np.array([0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=bool), np.array([0, 0, 0, 1, 0, 0, 0, 0, 1], dtype=bool)
    assert np.array_equal(p[0, 0], e[1:, 0][:, pos].sum(axis=1)) and np.array_equal(p[0, 1], e[1:, 0][:, neg].sum(axis=1))
    p0 = T.profiles(e, [0], 0.0, dtype=np.float64)                                             # THR == 0: 0.0, -0.0 and NaN count on neither side
    on = ~np.isin(np.arange(n), [4, 5, 6])
    assert np.array_equal(p0[0, 0], e[1:, 0][:, on & (e[0, 0] > 0)].sum(axis=1))
    assert np.array_equal(p0[0, 1], e[1:, 0][:, on & (e[0, 0] < 0)].sum(axis=1))
    k = T.pick(e, [0, 0, 0, 0], THR, [0.0, UP - THR, 5.0, NAN])
    assert np.array_equal(k[0], np.concatenate([[0.0], np.zeros(NP)]))                         # the first path of the band; tangent zero
    assert np.array_equal(k[1], np.concatenate([[2.0], e[1:, 0, 2]]))
    assert np.array_equal(k[2], np.concatenate([[-1.0], np.zeros(NP)])) and k[3, 0] == -1.0    # not there; NaN equals nothing
    dup = _expo([1.0, 2.0, 1.0, -0.0, 0.0])
    k = T.pick(dup, [0, 0], 0.0, [1.0, 0.0])
    assert k[0, 0] == 0.0 and np.array_equal(k[0, 1:], dup[1:, 0, 0])                          # the smaller index wins
    assert k[1, 0] == 3.0 and np.array_equal(k[1, 1:], dup[1:, 0, 3])                          # -0.0 == 0.0
