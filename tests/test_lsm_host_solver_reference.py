"""The host normal-equation solvers (mcx.plan.solve_normal_equations / solve_normal_equations_batch: the oracle path's solve and
the fallback of a device solve that flags a singular system) at every basis size K = 1..6 and exercise-state count S = 1..8,
against the normal equations and the back-transformation solved in mpmath at 50 digits (tests/lsm_reference.py).

One bound for every case: |c - c_ref|_inf <= C cond(G) eps ||T||_inf ||b_ref||_inf per state, cond(G) from mpmath, T the
back-transformation (the identity for the z-basis check at shift = 0, scale = 1)."""
import numpy as np
import pytest

import lsm_reference as R
from mcx import _abi
from mcx.plan import solve_normal_equations, solve_normal_equations_batch

C = 4.0
KS = [(K, S) for K in range(1, _abi.MAX_BASIS + 1) for S in range(1, _abi.MAX_STATES + 1)]


@pytest.mark.parametrize("K,S", KS, ids=[f"K{K}-S{S}" for K, S in KS])
def test_host_solvers_against_mpmath(K, S):
    ms, shifts, scales = [], [], []
    for kind in R.SPREADS:
        m, shift, scale = R.synthetic_moments(K, S, kind)
        got = solve_normal_equations(m, K, S, shift, scale, False, 0.0)
        R.check_solution(got, m, K, S, shift, scale, C, (K, S, kind))
        zb = solve_normal_equations(m, K, S, 0.0, 1.0, False, 0.0)
        R.check_solution(zb, m, K, S, 0.0, 1.0, C, (K, S, kind, "z"))
        ms.append(m); shifts.append(shift); scales.append(scale)
    # the batched solver on the same systems (plus a degenerate and an empty one in between)
    n = len(ms)
    deg_m = ms[0].copy()
    empty = np.zeros_like(ms[0])
    M = np.stack(ms + [deg_m, empty])
    deg = np.array([False] * n + [True, False])
    x0 = np.array([0.0] * n + [1.7, 0.0])
    out = solve_normal_equations_batch(M, K, S, np.array(shifts + [1.7, 0.0]), np.array(scales + [1.0, 1.0]), deg, x0)
    for q in range(n):
        R.check_solution(out[q], ms[q], K, S, shifts[q], scales[q], C, (K, S, "batch", q))
    v = np.array([1.7 ** k for k in range(K)])
    for s in range(S):
        want = v * (deg_m[(2 * K - 1) + s * K] / deg_m[0]) / (v @ v)
        assert np.allclose(out[n][s], want, rtol=4 * K * R.EPS, atol=0.0), (K, S, out[n][s], want)
    assert not out[n + 1].any()
    assert np.array_equal(out[n], solve_normal_equations(deg_m, K, S, 1.7, 1.0, True, 1.7))
    assert not solve_normal_equations(empty, K, S, 0.0, 1.0, False, 0.0).any()


@pytest.mark.parametrize("K", range(2, _abi.MAX_BASIS + 1))
def test_host_solver_exactly_singular_gram_matrix(K):
    """one distinct z and degenerate = 0: G has rank 1; np.linalg.solve raises and the host solver takes lstsq, whose
    minimum-norm solution is the one of the degenerate branch (v mean(Y) / (v.v) with v = [z^k])"""
    z = np.full(64, 0.5)
    Y = np.stack([np.full(64, 2.0 + s) for s in range(3)])
    m, _ = R.moments_ref(z, Y, K)
    got = solve_normal_equations(m, K, 3, 0.0, 1.0, False, 0.0)
    v = np.array([0.5 ** k for k in range(K)])
    for s in range(3):
        assert np.allclose(got[s], v * (2.0 + s) / (v @ v), rtol=1e-12, atol=1e-14), (K, s, got[s])
