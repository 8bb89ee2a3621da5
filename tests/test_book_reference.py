"""The long-double interpreter of the book program (tests/book_reference.py) against the CPU oracle, on every book of
tests/book_cases.py at n = 4099: orc_eval_book and orc_resolve_atoms within TOL_ORACLE of the reference per entry, relative to the
entry's magnitude M; the same exercise decision wherever the reference's margin lies outside the tie band; at most 1e-4 of the
paths tied.  TOL_ORACLE is four times the largest ratio |oracle - reference| / M these books show (each test prints its own)."""
import numpy as np
import pytest
import torch

import book_cases as BC
import book_reference as R

N = 4099
SEED = 77


def test_erf_against_mpmath():
    import mpmath
    mpmath.mp.prec = 100
    xs = np.concatenate([np.linspace(-7.0, 7.0, 57), [1e-300, 1e-8, 0.0, 0.5, 5.9, 6.6, 30.0]])
    got = R.erf_ld(xs)
    for x, g in zip(xs, got):
        ref = mpmath.erf(mpmath.mpf(float(x)))
        hi = float(g)
        g_mp = mpmath.mpf(hi) + mpmath.mpf(float(g - R.LD(hi)))          # the long double as a 100-bit number
        assert abs(g_mp - ref) <= mpmath.mpf(2) ** -60 * abs(ref), x


@pytest.mark.parametrize("name,expo_only", BC.REFERENCE_BOOKS, ids=[f"{b}{'-expo' if e else ''}" for b, e in BC.REFERENCE_BOOKS])
def test_oracle_against_the_long_double_reference(name, expo_only, oracle):
    b = BC.Book(name, oracle, expo_only)
    plan = b.plan
    paths = oracle.generate_paths(b.sc._sim, SEED, 0, N)
    R.nan_unused_rows(paths, b.used_rows())
    ref = R.evaluate(plan, paths.numpy(), band=R.TIE_BAND * R.TOL_ORACLE)
    bits = oracle.new_exercise_bits(len(plan.events), N)
    oracle.book_set_exercise_replay(b.book, 1, bits)
    try:
        cfs, expo = oracle.eval_book(b.book, paths)
    finally:
        oracle.book_set_exercise_replay(b.book, 0, None)
    worst = 0.0
    if not expo_only:
        worst = max(worst, R.worst_ratio(cfs.numpy(), ref.cfs, ref.cfs_M, ref.cfs_tied))
    worst = max(worst, R.worst_ratio(expo.numpy(), ref.expo, ref.expo_M, ref.expo_tied))
    ids = np.arange(len(plan.atoms))
    av = oracle.resolve_atoms(b.book, ids, paths).numpy()
    used = [k for k in ids if plan.atoms[k]["col"] < 0 or (int(plan.atoms[k]["t_idx"]), int(plan.atoms[k]["col"])) in b.used_rows()]
    worst_atom = max(R.worst_ratio(av[k], *R.atom(plan, k, paths.numpy())) for k in used)
    tied = ref.cfs_tied.any(axis=0) | ref.expo_tied.any(axis=(0, 1))
    print(f"{name} expo_only={expo_only}: oracle/reference worst ratio {worst:.3e} (atoms {worst_atom:.3e}), tied paths {int(tied.sum())}")
    assert worst <= R.TOL_ORACLE and worst_atom <= R.TOL_ORACLE
    assert tied.mean() <= 1e-4
    # decisions: equal outside the band (a path tied at an earlier event of the product may be in another state: left out)
    for p_i, pr in enumerate(plan.products):
        seen_tie = np.zeros(N, dtype=bool)
        for q in range(int(pr["ev_begin"]), int(pr["ev_end"])):
            if q in ref.decisions:
                seen_tie |= ref.tie_at[q]
                got = (bits[q].numpy() & 1).astype(bool)
                assert np.array_equal(got[~seen_tie], ref.decisions[q][~seen_tie]), (name, q)
    if name in ("exercise", "exotic", "all"):
        # every final state of the FlexiCall (4) and of the Bermudan (2) on at least 1 % of the paths: the coefficient rows
        # coeffs + coeff_off + s K of the paths of one lane differ
        for p_i, pr in enumerate(plan.products):
            if pr["n_states"] > 1:
                assert (np.bincount(ref.final_state[p_i], minlength=int(pr["n_states"])) >= N // 100).all(), (name, p_i)


def test_replay_follows_the_bits(oracle):
    """the oracle replaying random bits against the reference replaying the same bits: no indicator, no tie allowance"""
    b = BC.Book("exercise", oracle)
    plan = b.plan
    paths = oracle.generate_paths(b.sc._sim, SEED + 1, 0, N)
    r = np.random.default_rng(5)
    bits = torch.from_numpy(r.integers(0, 2, (len(plan.events), N), dtype=np.uint8))
    b.set_coeffs(oracle, BC.perturbed_coeffs(b.sc, b.base_coeffs, seed=BC.COEFF_SEED + 1))
    ref = R.evaluate(plan, paths.numpy(), replay={q: bits[q].numpy().astype(bool) for q in range(len(plan.events))})
    oracle.book_set_exercise_replay(b.book, 2, bits)
    try:
        cfs, expo = oracle.eval_book(b.book, paths)
    finally:
        oracle.book_set_exercise_replay(b.book, 0, None)
    assert not ref.cfs_tied.any() and not ref.expo_tied.any()
    assert R.worst_ratio(cfs.numpy(), ref.cfs, ref.cfs_M) <= R.TOL_ORACLE
    assert R.worst_ratio(expo.numpy(), ref.expo, ref.expo_M) <= R.TOL_ORACLE
