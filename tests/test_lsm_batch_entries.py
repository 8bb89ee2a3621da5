"""Two properties of the LSM entry points that the host code behind them must keep, whoever shares it:

1. every batched K3 entry point (mcx_lsm_step_batch, mcx_lsm_step_batch_dev, mcx_lsm_run_batch, mcx_lsm_solve_batch) refuses, with
   code -2 and before any launch, each index of a job table that a kernel would dereference;
2. the two callers of the normal-equation solver (lsm_solve.h: k3_solve_t behind mcx_lsm_solve_batch, k6_solve_state behind
   mcx_storage_lsm_solve_batch) return the same bits for the same system."""
import numpy as np
import pytest
import torch

import cases
import lsm_reference as R
from mcx import _abi
from mcx._native import McxError

pytestmark = pytest.mark.gpu


# ---- 1. refusals ------------------------------------------------------------------------------------------------------------------
def test_batched_entry_points_refuse_bad_job_tables_before_any_launch(hip):
    """the irs_cva book (one product of one exercise state), one job.  After each refusal the cache (filled with a sentinel) and the
    book's coefficients are what they were, and so is the device flag of mcx_lsm_solve_batch (the flag of mcx_lsm_run_batch is a
    host word that the wrapper does not return when the call fails): nothing ran"""
    sc, _ = cases.make_controller("irs_cva", hip, inject=False)
    sc.prepare()
    plan = sc.book_plan
    paths = sc.last_state.get("paths_pre")
    if paths is None:
        paths = torch.zeros(sc.sim_plan.n_dates, sc.sim_plan.n_state, 1024, dtype=torch.float64, device=hip.device)
    n = paths.shape[2]
    W = hip.zeros(n).fill_(1.5)
    W2 = hip.zeros(2 * n).fill_(1.5)                                   # room for two states: the state check is what refuses
    before = hip.book_get_coeffs(sc.book).copy()
    K = plan.n_basis

    def tables():
        jobs = np.zeros(1, dtype=_abi.LSM_JOB_DTYPE)
        sj = np.zeros(1, dtype=_abi.LSM_SOLVE_JOB_DTYPE)
        sj["coeff_off"][:] = -1
        sj["scale"] = 1.0
        return jobs, sj

    def refused(call, words, who):
        with pytest.raises(McxError) as e:
            call()
        msg = hip.lib.mcx_last_error(hip.h).decode()
        assert e.value.code == -2 and words in msg and who in msg, (words, who, msg)
        hip.synchronize()
        assert (W == 1.5).all().item() and (W2 == 1.5).all().item(), (words, who)
        assert np.array_equal(hip.book_get_coeffs(sc.book), before), (words, who)

    bad_jobs = {"product out of range": ("product", len(plan.products), 1), "states": (None, None, 2),
                "roll window": ("roll_end", 10 ** 6, 1), "atoms": ("num_atom", len(plan.atoms), 1), "outside d_W": ("w_offset", 1, 1)}
    for words, (field, value, S) in bad_jobs.items():
        jobs, sj = tables()
        if field is not None:
            jobs[field] = value
        cache = W if S == 1 else W2
        refused(lambda: hip.lsm_step_batch(sc.book, jobs, S, paths, cache, n), words, "mcx_lsm_step_batch")
        refused(lambda: hip.lsm_step_batch_dev(sc.book, jobs, S, paths, cache, n), words, "mcx_lsm_step_batch")
        refused(lambda: hip.lsm_run_batch(sc.book, jobs, sj, np.array([0, 1]), np.array([S]), paths, cache, n), words, "mcx_lsm_run_batch")
    jobs, sj = tables()
    jobs["x_atom"] = -1                                                # (the other atom, below the range)
    refused(lambda: hip.lsm_step_batch(sc.book, jobs, 1, paths, W, n), "atoms", "mcx_lsm_step_batch")
    # a [1][K] coefficient block that ends beyond the array, in either slot
    for slot in (0, 1):
        jobs, sj = tables()
        sj["coeff_off"][0, slot] = len(plan.coeffs) - K + 1
        refused(lambda: hip.lsm_run_batch(sc.book, jobs, sj, np.array([0, 1]), np.array([1]), paths, W, n), "coefficient offset", "mcx_lsm_run_batch")
        flag = hip.zeros(1, dtype=torch.int32).fill_(7)
        mom = hip.zeros(1, (2 * K - 1) + K)
        refused(lambda: hip.lsm_solve_batch(sc.book, sj, 1, mom, flag), "coefficient offset", "mcx_lsm_solve_batch")
        assert int(flag.cpu()[0]) == 7
    # the step table of the one-call induction
    jobs, sj = tables()
    refused(lambda: hip.lsm_run_batch(sc.book, jobs, sj, np.array([1, 1]), np.array([1]), paths, W, n), "must start at job 0", "mcx_lsm_run_batch")
    refused(lambda: hip.lsm_run_batch(sc.book, jobs, sj, np.array([0, 2, 1]), np.array([1, 1]), paths, W, n), "not ascending", "mcx_lsm_run_batch")


# ---- 2. the two callers of the solver ---------------------------------------------------------------------------------------------------
def test_storage_and_exercise_solvers_return_the_same_bits(hip):
    """the first step of a book of three storages of 2, 7 and 4 states (K = 3, 257 paths, a random cache): its moments solved by
    mcx_storage_lsm_solve_batch (lane s of a block: state s) and by mcx_lsm_solve_batch with n_states = S (one lane: all states;
    <3,2> is a compile-time specialisation of k3_solve_t, (3,7) and (3,4) take its run-time bounds) into the same spare coefficient
    blocks.  A regular, a degenerate and a singular system; the singular one writes no coefficients on either side."""
    from test_storage_batch_gpu import Book
    K, n = 3, 257
    b = Book(hip, K, n, ((2, 3.0, 1.0), (7, 5.5, 2.0), (4, 4.0, 1.0)), (0.0, 1.0))
    S_of = b.S_of
    assert S_of == [2, 7, 4] and max(S_of) <= _abi.MAX_STATES and b.step_begin[1] == 3
    book = b.sc.book
    stride = (2 * K - 1) + max(S_of) * K
    step = np.ascontiguousarray(b.jobs[:3].copy(), dtype=_abi.STORAGE_LSM_JOB_DTYPE)
    assert step["storage"].tolist() == [0, 1, 2] and not step["degenerate"].any()      # (the explanatory variable varies over the paths)
    spare = np.concatenate([[0], np.cumsum(np.asarray(S_of) * K)])      # job j's spare block of the book's coefficients
    assert spare[-1] <= len(book.plan.coeffs)
    step["coeff_off"][:, 0], step["coeff_off"][:, 1] = spare[:3], -1
    b.reset()
    before = hip.book_get_coeffs(book).copy()
    W = hip.from_numpy(np.random.default_rng(5).uniform(0.0, 10.0, b.w_len))
    mom = hip.storage_lsm_step_batch(book, b.handles, step, b.paths, W, n, stride)
    z = np.full(200, 0.5)                                              # one distinct z: a Gram matrix of rank 1
    singular = np.zeros((3, stride))
    for j, S in enumerate(S_of):
        ms, _ = R.moments_ref(z, np.stack([np.full(200, 1.0 + s) for s in range(S)]), K)
        singular[j, :len(ms)] = ms
    systems = {"regular": (mom, 0, 0), "degenerate": (mom, 1, 0), "singular": (hip.from_numpy(singular), 0, 1)}
    for tag, (m, degenerate, want_status) in systems.items():
        jobs = step.copy()
        jobs["degenerate"], jobs["x0"] = degenerate, 1.3
        # the storage's solver: the packed table and the spare blocks
        b.reset()
        table = hip.zeros(int(spare[-1])).fill_(3.5)
        status = hip.zeros(3, dtype=torch.int32).fill_(7)
        hip.storage_lsm_solve_batch(book, b.handles, jobs, m, table, status)
        tab, st = table.cpu().numpy(), status.cpu().numpy()
        co6 = hip.book_get_coeffs(book).copy()
        assert st.tolist() == [want_status] * 3, (tag, st)
        # the exercise products' solver: job by job (their state counts differ)
        b.reset()
        for j, S in enumerate(S_of):
            sj = np.zeros(1, dtype=_abi.LSM_SOLVE_JOB_DTYPE)
            for f in ("shift", "scale", "x0", "degenerate"):
                sj[f] = jobs[f][j]
            sj["coeff_off"][0] = (spare[j], -1)
            flag = hip.zeros(1, dtype=torch.int32)
            hip.lsm_solve_batch(book, sj, S, m[j:j + 1, :(2 * K - 1) + S * K].contiguous(), flag)
            assert int(flag.cpu()[0]) == want_status, (tag, j)
        co3 = hip.book_get_coeffs(book).copy()
        if want_status:
            assert np.array_equal(co6, before) and np.array_equal(co3, before), tag
            continue
        assert np.array_equal(co6[:spare[-1]], tab) and np.array_equal(co6[spare[-1]:], before[spare[-1]:]), tag
        assert np.isfinite(tab).all() and tab.any() and not np.array_equal(tab, before[:spare[-1]]), tag
        assert np.array_equal(co3, co6), (tag, np.abs(co3 - co6).max(), co3[:spare[-1]], co6[:spare[-1]])
    b.reset()
