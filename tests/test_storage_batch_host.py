"""The job table of the product-batched storage induction (mcx.controller.controller.storage_lsm_job_table), on the host alone:
three made-up schedules of lengths 5, 3 and 1, some entries without a roll.  No backend, no library."""
from mcx import _abi
from mcx.controller.controller import storage_lsm_dates, storage_lsm_job_table

K, LD_W = 3, 10
S_OF = [4, 2, 7]
REG_BASE, EXPO_BASE = [1000, 2000, 3000], [5000, 6000, 7000]
# (t_reg, r0, r1, prod_idx, expo_idx): r1 == r0 is a step without a roll; a date may feed the product block, an exposure row or both
SCHEDS = [
    [(4.0, 4, 5, 4, None), (3.5, 4, 4, None, 3), (3.0, 3, 4, 3, 2), (2.0, 2, 3, 2, None), (0.0, 0, 1, 0, 0)],
    [(2.0, 2, 2, None, 2), (1.0, 1, 2, 1, None), (0.0, 0, 1, 0, 0)],
    [(0.0, 0, 0, None, 0)],
]
ATOMS = [[(10 + r, 24 - r) for r in range(5)], [(30 + r, 40 + r) for r in range(3)], [(50, 20)]]
X_RANGE = {20: (30.0, 30.0), **{20 + r: (25.0 - r, 40.0 + r) for r in range(1, 5)}, **{40 + r: (1.0, 2.0 + r) for r in range(3)}}


def _table():
    dates_of = [storage_lsm_dates(S_OF[j], K, SCHEDS[j], ATOMS[j], X_RANGE, REG_BASE[j], EXPO_BASE[j]) for j in range(3)]
    return dates_of, storage_lsm_job_table(dates_of, S_OF, LD_W)


def test_step_begin_and_product_order():
    _, (jobs, step_begin, job_of, w_len) = _table()
    assert jobs.dtype == _abi.STORAGE_LSM_JOB_DTYPE
    assert step_begin.tolist() == [0, 3, 5, 7, 8, 9] and len(jobs) == 9
    per_step = [jobs["storage"][step_begin[t]:step_begin[t + 1]].tolist() for t in range(5)]
    # each storage at most once per step, in product order; the last steps hold one job
    assert per_step == [[0, 1, 2], [0, 1], [0, 1], [0], [0]]
    assert [d.tolist() for d in job_of] == [[0, 3, 5, 7, 8], [1, 4, 6], [2]]
    assert w_len == 2 * LD_W * sum(S_OF)


def test_cache_halves_alternate_only_on_rolls_inside_the_storages_own_block():
    dates_of, (jobs, step_begin, job_of, w_len) = _table()
    base = 0
    for j in range(3):
        blk = S_OF[j] * LD_W
        lo, hi = base, base + 2 * blk
        cur = lo                                                    # the half that holds the cache: the first one at the start
        for r, k in enumerate(job_of[j]):
            q = jobs[k]
            assert q["w_old"] == cur, (j, r)
            assert q["w_old"] in (lo, lo + blk) and q["w_new"] in (lo, lo + blk) and q["w_new"] != q["w_old"]
            assert lo <= q["w_old"] and q["w_old"] + blk <= hi and lo <= q["w_new"] and q["w_new"] + blk <= hi
            rolls = SCHEDS[j][r][2] > SCHEDS[j][r][1]
            assert (q["roll_date"] >= 0) == rolls and (not rolls or q["roll_date"] == SCHEDS[j][r][1])
            if rolls:
                cur = q["w_new"]
        base = hi
    assert base == w_len
    assert [int((d["roll_date"] >= 0).sum()) for d in dates_of] == [4, 2, 0]     # the table above does hold steps without a roll


def test_jobs_carry_what_the_per_storage_route_would_write():
    """every field the two routes share equals the per-storage date table (what _storage_regression hands to mcx_storage_lsm_run),
    and the coefficient targets are the product / exposure blocks of the schedule entry"""
    dates_of, (jobs, step_begin, job_of, w_len) = _table()
    for j in range(3):
        SK = S_OF[j] * K
        for r, k in enumerate(job_of[j]):
            q, d = jobs[k], dates_of[j][r]
            for f in ("roll_date", "num_atom", "x_atom", "degenerate", "shift", "scale", "x0"):
                assert q[f] == d[f], (j, r, f)
            _, _, _, prod_idx, expo_idx = SCHEDS[j][r]
            want = [-1 if prod_idx is None else REG_BASE[j] + prod_idx * SK, -1 if expo_idx is None else EXPO_BASE[j] + expo_idx * SK]
            assert q["coeff_off"].tolist() == want == d["coeff_off"].tolist()
            assert (q["num_atom"], q["x_atom"]) == ATOMS[j][r]
    # the calibration date of storage 0 and the only date of storage 2 regress on atom 20, whose range is one point
    assert jobs[job_of[0][4]]["degenerate"] == 1 and jobs[job_of[2][0]]["degenerate"] == 1
    q = jobs[job_of[0][4]]
    assert (q["shift"], q["scale"], q["x0"]) == (30.0, 1.0, 30.0)
    q = jobs[job_of[1][1]]                                          # x in [1, 3]: centred and scaled to [-1, 1]
    assert (q["degenerate"], q["shift"], q["scale"], q["x0"]) == (0, 2.0, 1.0, 1.0)


def test_an_empty_book_of_storages_gives_an_empty_table():
    jobs, step_begin, job_of, w_len = storage_lsm_job_table([], [], LD_W)
    assert len(jobs) == 0 and step_begin.tolist() == [0] and job_of == [] and w_len == 0
