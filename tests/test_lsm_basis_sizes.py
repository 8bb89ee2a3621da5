"""The regression kernels at every basis size K = 1..6 (PolyomialRegression(degree = K - 1)) and exercise-state count S = 1..8.

A. k3_step_valu / k3_step_mfma / k3_step_batch: the rolled cashflow cache against the CPU oracle on the same paths and
   coefficients (same exercise decision on every path and state), the moments against an exact sum rebuilt from the kernel's
   own rolled cache: |m - m_ref| <= C_MOM (2K + log2 n) eps sum|term|.
B. the device solvers (mcx_lsm_solve, mcx_lsm_run, mcx_lsm_solve_batch, mcx_lsm_run_batch: k3_solve_t's specialisations and
   its run-time-bound <0,0> path) against mpmath: |c - c_ref| <= C_SOLVE cond(G) eps ... (tests/lsm_reference.py), and the
   degenerate, empty and singular branches against their definitions.
C. whole runs against the oracle at degrees other than 2: exercise products, FlexiCalls of 4..7 rights, a CVA book off the
   CVA fast paths and a large book through the product-batched induction.
D. forward-mode sensitivities through kt_lsm<1,2,4> / kt_lsm_step<2,2> / <4,2> against replayed bumps, and the configurations
   without a tangent form falling back to bumps.
The last test checks that the module reached every instantiation it claims (SEEN, recorded by the thin wrappers below).
The reference anchors away from K = 3 (a Bermudan swaption at degree 3, a 5-right FlexiCall at degree 1: the reference's
torch.linalg.lstsq on raw monomials) are cases of tests/cases.py (REGRESSION_DEGREE), pinned by test_oracle_golden.py (CPU
oracle) and test_hip_parity.py (HIP inject-Z)."""
import math

import numpy as np
import pytest
import torch

import cases
import lsm_reference as R
from mcx import _abi
from mcx.maths.regression import PolyomialRegression

pytestmark = pytest.mark.gpu

KMAX, SMAX = _abi.MAX_BASIS, _abi.MAX_STATES
KS = [(K, S) for K in range(1, KMAX + 1) for S in range(1, SMAX + 1)]
KS_IDS = [f"K{K}-S{S}" for K, S in KS]
SMALL_N = (0, 1, 63, 65, 4095, 20011)
C_MOM = 4.0
C_SOLVE = 4.0
SOLVE_SPECS = {(2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (4, 1), (4, 2)}      # k3_solve_body's compile-time (K, S); else <0,0>
SEEN = {"step": set(), "solve": set(), "kt_lsm": set(), "kt_lsm_step": set()}


def _solve_spec(K, S):
    return (K, S) if (K, S) in SOLVE_SPECS else (0, 0)


# ---- books ------------------------------------------------------------------------------------------------------------------
def _flexi_book(S, n_rights=None, model=None):
    """Black-Scholes FlexiCall of S - 1 rights on S + 1 puts (S exercise states), PV + EPE"""
    model = model or cases.BlackScholesModel(0, 100.0, 0.03, 0.25)
    L = S + 1
    opts = [cases.EuropeanOption(cases.Equity(), 0.125 * (k + 1), 97.0 + 1.5 * k, cases.OptionType.PUT) for k in range(L)]
    fc = cases.FlexiCall(opts, S - 1 if n_rights is None else n_rights)
    fc.name = "flexi"
    tl = np.linspace(0.0, 0.125 * L, L + 1)
    return [cases.NettingSet(name="flexi", products=[fc])], model, cases.RiskMetrics([cases.PVMetric(), cases.EPEMetric()], exposure_timeline=tl)


def _controller(K, S, be, n_main=1024, n_pre=1024):
    if S == 1:
        ns, model, rm = cases.irs_cva()            # a payer swap: S = 1, regressed exposures
        steps, scheme = 2, cases.E
    else:
        ns, model, rm = _flexi_book(S)
        steps, scheme = 1, cases.A
    return cases.SimulationController(ns, model, rm, n_main, n_pre, steps, scheme, backend=be,
                                      regression_function=PolyomialRegression(degree=K - 1))


class _Ctx:
    """one compiled (K, S) book: the HIP book, an oracle book on the same plan, the regression step with the widest roll window"""

    def __init__(self, K, S, hip, oracle):
        self.K, self.S = K, S
        sc = _controller(K, S, hip)
        sc.prepare()
        assert sc.book_plan.n_basis == K
        self.sc, self.book, self.obook = sc, sc.book, oracle.book_create(sc.book_plan)
        p = sc.products[0]
        assert p.get_num_states() == S
        sched = sc._regression_schedule(0, p)
        atoms = sc._regression_atoms(sched, p.asset_ids[0])
        j = int(np.argmax([r1 - r0 for (_t, r0, r1, _a, _b) in sched]))
        self.r0, self.r1 = sched[j][1], sched[j][2]
        self.num, self.x = atoms[j]
        assert self.r1 > self.r0
        # non-trivial continuation coefficients (the regression's own, perturbed) in both books
        c = hip.book_get_coeffs(self.book)
        r = np.random.default_rng(K * 16 + S)
        self.coeffs = c * (1.0 + 0.05 * r.standard_normal(c.shape)) + 0.01 * r.standard_normal(c.shape)
        hip.book_set_coeffs(self.book, 0, self.coeffs)          # (writes the shared plan's array the oracle reads too)
        assert np.array_equal(sc.book_plan.coeffs, self.coeffs)
        self.n_coeffs = len(c)
        self.n_events = len(sc.book_plan.events)


_CTX = {}


@pytest.fixture(scope="module")
def ctx(hip, oracle):
    def get(K, S):
        if (K, S) not in _CTX:
            _CTX[(K, S)] = _Ctx(K, S, hip, oracle)
        return _CTX[(K, S)]
    yield get
    _CTX.clear()


def _paths(hip, c, n, seed=11):
    """[dates][state][n] pre-simulation paths; n = 0: a one-path tensor narrowed by _Empty (an empty torch tensor has no data
    pointer, and the library rejects null pointers before it looks at the path count)"""
    if n == 0:
        return _Empty(hip.generate_paths(c.sc._sim, seed, 0, 1))
    return hip.generate_paths(c.sc._sim, seed, 0, n)


class _Empty:
    """a paths tensor of zero paths with a valid device pointer: shape [T][D][0], the buffer of a one-path tensor"""

    def __init__(self, t):
        self.t = t
        self.shape = (t.shape[0], t.shape[1], 0)

    def data_ptr(self):
        return self.t.data_ptr()

    def stride(self, k=None):
        return self.t.stride() if k is None else self.t.stride(k)

    def dim(self):
        return 3

    def cpu(self):
        return self.t.cpu()[..., :0]


def _shift_scale(hip, c, paths):
    n = paths.shape[2]
    if n == 0:
        return 0.0, 1.0
    x = hip.resolve_atoms(c.book, [c.x], paths)[0].cpu().numpy()
    lo, hi = float(x.min()), float(x.max())
    return (0.5 * (lo + hi), 2.0 / (hi - lo)) if hi > lo else (lo, 1.0)


# ---- thin wrappers: every device call of A / B goes through these and is recorded ---------------------------------------------
def _step(hip, c, paths, W, shift, scale, flags):
    m = hip.lsm_step(c.book, 0, c.r0, c.r1, c.num, c.x, shift, scale, paths, W, flags=flags)
    SEEN["step"].add(("mfma" if flags & _abi.LSM_MFMA else "valu", c.K, c.S))
    return m.cpu().numpy()


def _step_batch(hip, c, jobs, paths, W, ld_w, flags=0):
    m = hip.lsm_step_batch(c.book, jobs, c.S, paths, W, ld_w, flags=flags)
    SEEN["step"].add(("batch", c.K, c.S))
    return m


def _record_solve(entry, K, S):
    SEEN["solve"].add((entry, _solve_spec(K, S)))


# ---- A: moment kernels ------------------------------------------------------------------------------------------------------
def _check_moments(hip, c, paths, W_after, shift, scale, mom, tag):
    K, S = c.K, c.S
    n = paths.shape[2]
    NM = (2 * K - 1) + S * K
    assert mom.shape == (NM,), (tag, mom.shape)
    if n == 0:
        assert not mom.any(), (tag, mom)
        return
    a = hip.resolve_atoms(c.book, [c.num, c.x], paths).cpu().numpy()       # the kernel's own dev_atom values
    num, x = a[0], a[1]
    z = (x - shift) * scale
    Y = num[None, :] * W_after[:, :n]
    ref, mag = R.moments_ref(z, Y, K)
    bound = C_MOM * (2 * K + math.log2(max(n, 2))) * R.EPS * mag
    err = np.abs(mom - ref)
    assert (err <= bound).all(), (tag, np.nonzero(err > bound)[0], mom, ref, err / np.maximum(bound, 1e-300))


def _roll_against_oracle(hip, oracle, c, n, flags, seed=11):
    """one lsm_step on HIP and on the oracle from the same W; -> (paths, rolled W, moments, shift, scale) after the checks of the
    roll (W to 1e-12, identical exercise decisions) and of the moments"""
    paths = _paths(hip, c, n, seed)
    shift, scale = _shift_scale(hip, c, paths)
    r = np.random.default_rng(n + 7 * c.K + 131 * c.S)
    W0 = r.uniform(0.0, 10.0, (c.S, max(n, 1)))
    Wh = hip.from_numpy(W0.copy())
    Wo = torch.from_numpy(W0.copy())
    pc = paths.cpu().contiguous()
    if n:
        bh, bo = hip.new_exercise_bits(c.n_events, n), oracle.new_exercise_bits(c.n_events, n)
        hip.book_set_exercise_replay(c.book, 1, bh)
        oracle.book_set_exercise_replay(c.obook, 1, bo)
    try:
        mom = _step(hip, c, paths, Wh, shift, scale, flags)
        if n:                                      # (zero paths: nothing rolls, W must come back unchanged)
            oracle.lsm_step(c.obook, 0, c.r0, c.r1, c.num, c.x, shift, scale, pc, Wo, flags=flags & _abi.LSM_F32_CACHE)
    finally:
        if n:
            hip.book_set_exercise_replay(c.book, 0, None)
            oracle.book_set_exercise_replay(c.obook, 0, None)
    Wg = Wh.cpu().numpy()
    tag = (c.K, c.S, n, flags)
    if n:
        assert np.array_equal(bh.cpu().numpy(), bo.numpy()), (tag, "exercise decisions differ")
        if c.S > 1 and n >= 4095:                  # the roll took exercise branches both ways (bit s: decision in state s > 0)
            bits = bo.numpy()
            mask = ((1 << c.S) - 1) & ~1
            rows = bits[(bits != 0).any(axis=1)]
            assert len(rows) and ((rows & mask) != mask).any(), tag
    scale_w = max(np.abs(Wo.numpy()).max(), 1e-300)
    assert np.allclose(Wg, Wo.numpy(), rtol=1e-12, atol=1e-12 * scale_w), (tag, np.abs(Wg - Wo.numpy()).max())
    _check_moments(hip, c, paths, Wg, shift, scale, mom, tag)
    return paths, Wg, Wo.numpy(), mom


def _batch_against_oracle(hip, oracle, c, n, n_jobs=5, seed=23):
    """one lsm_step_batch of n_jobs jobs of the product (their own cache blocks, shifts and scales, two roll windows) against the
    oracle's composition of lsm_step"""
    K, S = c.K, c.S
    paths = _paths(hip, c, n, seed)
    shift, scale = _shift_scale(hip, c, paths)
    sched = c.sc._regression_schedule(0, c.sc.products[0])
    wins = sorted({(r0, r1) for (_t, r0, r1, _a, _b) in sched if r1 > r0}, key=lambda w: w[0] - w[1])
    ld_w = n
    jobs = np.zeros(n_jobs, dtype=_abi.LSM_JOB_DTYPE)
    for j in range(n_jobs):
        r0, r1 = wins[j % len(wins)] if j % 2 == 0 else (c.r0, c.r1)
        jobs[j]["product"], jobs[j]["roll_begin"], jobs[j]["roll_end"] = 0, r0, r1
        jobs[j]["num_atom"], jobs[j]["x_atom"] = c.num, c.x
        jobs[j]["w_offset"] = j * S * ld_w
        jobs[j]["shift"], jobs[j]["scale"] = shift + 0.01 * j, scale * (1.0 + 0.1 * j)
    r = np.random.default_rng(n + K + 17 * S)
    W0 = r.uniform(0.0, 10.0, n_jobs * S * ld_w)
    Wh, Wo = hip.from_numpy(W0.copy()), torch.from_numpy(W0.copy())
    mom = _step_batch(hip, c, jobs, paths, Wh, ld_w)
    oracle.lsm_step_batch(c.obook, jobs, S, paths.cpu().contiguous(), Wo, ld_w)
    Wg = Wh.cpu().numpy()
    scale_w = max(np.abs(Wo.numpy()).max(), 1e-300)
    assert np.allclose(Wg, Wo.numpy(), rtol=1e-12, atol=1e-12 * scale_w), (K, S, n, np.abs(Wg - Wo.numpy()).max())
    for j in range(n_jobs):
        blk = Wg[j * S * ld_w:(j + 1) * S * ld_w].reshape(S, ld_w)
        _check_moments(hip, c, paths, blk, float(jobs[j]["shift"]), float(jobs[j]["scale"]), mom[j], (K, S, n, "batch", j))


@pytest.mark.parametrize("K,S", KS, ids=KS_IDS)
def test_moment_kernels_at_small_path_counts(K, S, ctx, hip, oracle):
    c = ctx(K, S)
    for n in SMALL_N:
        for flags in (0, _abi.LSM_MFMA):
            _roll_against_oracle(hip, oracle, c, n, flags)
    for n in (65, 4095):
        _batch_against_oracle(hip, oracle, c, n)


BIG_KS = [(1, 1), (6, 8), (3, 2), (2, 5), (5, 3), (4, 7)]


@pytest.mark.parametrize("K,S", BIG_KS, ids=[f"K{K}-S{S}" for K, S in BIG_KS])
def test_moment_kernels_on_the_grid_stride_loop(K, S, ctx, hip, oracle):
    """more paths than 4 n_cu blocks of 256 lanes: the grid-stride loop of the VALU kernel, MFMA's iters / live logic on a ragged
    last iteration, several paths per lane in the batch kernel"""
    c = ctx(K, S)
    n = 4 * hip.device_info()["n_cu"] * 256 + 4097
    for flags in (0, _abi.LSM_MFMA):
        _roll_against_oracle(hip, oracle, c, n, flags, seed=5)
    _batch_against_oracle(hip, oracle, c, n, n_jobs=4, seed=6)


def test_float32_cache_roll_is_bit_identical_to_the_oracle(ctx, hip, oracle):
    c = ctx(KMAX, SMAX)
    _, Wg, Wo, _ = _roll_against_oracle(hip, oracle, c, 20011, _abi.LSM_F32_CACHE)
    assert np.array_equal(Wg, Wo)


# ---- B: device solvers ------------------------------------------------------------------------------------------------------
def _date(c, shift, scale, off0, off1, degenerate=0, x0=0.0, window=None):
    d = np.zeros(1, dtype=_abi.LSM_DATE_DTYPE)
    r0, r1 = window if window is not None else (0, 0)
    d["roll_begin"], d["roll_end"], d["num_atom"], d["x_atom"], d["degenerate"] = r0, r1, c.num, c.x, degenerate
    d["coeff_off"][0, 0], d["coeff_off"][0, 1] = off0, off1
    d["shift"], d["scale"], d["x0"] = shift, scale, x0
    return d


def _blocks(c, n):
    SK = c.S * c.K
    assert c.n_coeffs >= n * SK, (c.K, c.S, c.n_coeffs)
    return [q * SK for q in range(n)]


def _solve_one(hip, c, m, shift, scale, off0=-1, off1=-1, degenerate=0, x0=0.0):
    tab = hip.zeros(c.S * c.K)
    st = hip.zeros(1, dtype=torch.int32)
    hip.lsm_solve(c.book, 0, hip.from_numpy(np.ascontiguousarray(m)), _date(c, shift, scale, off0, off1, degenerate, x0), 0, tab, st)
    _record_solve("solve", c.K, c.S)
    return tab.cpu().numpy().reshape(c.S, c.K), int(st.cpu()[0])


def _solve_batch(hip, c, ms, shifts, scales, offs, degenerate=None, x0=None):
    n = len(ms)
    sj = np.zeros(n, dtype=_abi.LSM_SOLVE_JOB_DTYPE)
    sj["shift"], sj["scale"] = shifts, scales
    sj["coeff_off"][:, 0], sj["coeff_off"][:, 1] = offs, -1
    sj["degenerate"] = 0 if degenerate is None else degenerate
    sj["x0"] = 0.0 if x0 is None else x0
    flag = hip.zeros(1, dtype=torch.int32)
    hip.lsm_solve_batch(c.book, sj, c.S, hip.from_numpy(np.ascontiguousarray(np.stack(ms))), flag)
    _record_solve("solve_batch", c.K, c.S)
    co = hip.book_get_coeffs(c.book)
    return [co[o:o + c.S * c.K].reshape(c.S, c.K) for o in offs], int(flag.cpu()[0])


@pytest.mark.parametrize("K,S", KS, ids=KS_IDS)
def test_device_solvers_against_mpmath(K, S, ctx, hip):
    c = ctx(K, S)
    offs = _blocks(c, 2 * len(R.SPREADS))
    hip.book_set_coeffs(c.book, 0, c.coeffs)
    cases_ = []
    for kind in R.SPREADS:
        m, shift, scale = R.synthetic_moments(K, S, kind)
        cases_ += [(m, shift, scale, kind), (m, 0.0, 1.0, kind + "/z")]
    # mcx_lsm_solve: the result table and both coefficient slots
    for q, (m, shift, scale, tag) in enumerate(cases_):
        tab, st = _solve_one(hip, c, m, shift, scale, off0=offs[q], off1=offs[(q + 1) % len(offs)])
        assert st == 0, (K, S, tag)
        R.check_solution(tab, m, K, S, shift, scale, C_SOLVE, (K, S, "solve", tag))
        co = hip.book_get_coeffs(c.book)
        for o in (offs[q], offs[(q + 1) % len(offs)]):
            assert np.array_equal(co[o:o + S * K].reshape(S, K), tab), (K, S, tag)
    # mcx_lsm_solve_batch: all systems in one launch
    hip.book_set_coeffs(c.book, 0, c.coeffs)
    got, flag = _solve_batch(hip, c, [x[0] for x in cases_], [x[1] for x in cases_], [x[2] for x in cases_], offs)
    assert flag == 0
    for (m, shift, scale, tag), g in zip(cases_, got):
        R.check_solution(g, m, K, S, shift, scale, C_SOLVE, (K, S, "solve_batch", tag))
    hip.book_set_coeffs(c.book, 0, c.coeffs)


def _run_inputs(hip, c, n, kind):
    """paths, a synthetic cache W [S][n] and (shift, scale) for the run entries with an empty roll window: the moments are those
    of z = (x - shift) scale and Y = num W on the pre-simulation paths"""
    paths = _paths(hip, c, n, seed=31)
    x = hip.resolve_atoms(c.book, [c.num, c.x], paths).cpu().numpy()
    lo, hi = float(x[1].min()), float(x[1].max())
    shift, scale = {"well": (0.5 * (lo + hi), 2.0 / (hi - lo)), "clustered": (lo - 2.0 * (hi - lo), 1.0 / (hi - lo)),
                    "shifted": (lo - 0.5 * (hi - lo), 0.5 / (hi - lo))}[kind]
    r = np.random.default_rng(c.K * 8 + c.S + len(kind))
    xs = (x[1] - lo) / (hi - lo)
    W = np.stack([np.maximum(xs - 0.2 * s / c.S, 0.0) + 0.1 * r.standard_normal(n) for s in range(c.S)])
    z = (x[1] - shift) * scale
    m, mag = R.moments_ref(z, x[0][None, :] * W, c.K)
    return paths, W, shift, scale, m, (2 * c.K + math.log2(n))


@pytest.mark.parametrize("K,S", KS, ids=KS_IDS)
def test_device_run_entries_against_mpmath(K, S, ctx, hip):
    """mcx_lsm_run (k3_finish_solve) and mcx_lsm_run_batch (k3_finish_solve_batch) on pre-simulation paths: moments and solve in
    one call each; the reference solves the exact moments, the bound carries the moments' own rounding"""
    c = ctx(K, S)
    n = 3001
    offs = _blocks(c, len(R.SPREADS))
    inputs = [_run_inputs(hip, c, n, kind) for kind in R.SPREADS]
    for q, (paths, W, shift, scale, m, mom_err) in enumerate(inputs):
        Wd = hip.from_numpy(W.copy())
        coeffs, status = hip.lsm_run(c.book, 0, _date(c, shift, scale, offs[q], -1), paths, Wd)
        _record_solve("run", K, S)
        assert status[0] == 0, (K, S, q)
        R.check_solution(coeffs[0], m, K, S, shift, scale, C_SOLVE, (K, S, "run", R.SPREADS[q]), moment_err=mom_err)
        assert np.array_equal(hip.book_get_coeffs(c.book)[offs[q]:offs[q] + S * K].reshape(S, K), coeffs[0])
    # the same systems as one batched step of three jobs (own cache blocks, shift / scale per job)
    hip.book_set_coeffs(c.book, 0, c.coeffs)
    paths = inputs[0][0]
    jobs = np.zeros(len(inputs), dtype=_abi.LSM_JOB_DTYPE)
    sj = np.zeros(len(inputs), dtype=_abi.LSM_SOLVE_JOB_DTYPE)
    Wflat = np.concatenate([inp[1].reshape(-1) for inp in inputs])
    for q, (_p, _W, shift, scale, _m, _e) in enumerate(inputs):
        jobs[q]["product"], jobs[q]["num_atom"], jobs[q]["x_atom"], jobs[q]["w_offset"] = 0, c.num, c.x, q * S * n
        jobs[q]["shift"], jobs[q]["scale"] = shift, scale
        sj[q]["shift"], sj[q]["scale"], sj[q]["coeff_off"] = shift, scale, (offs[q], -1)
    flag = hip.lsm_run_batch(c.book, jobs, sj, np.array([0, len(inputs)]), np.array([S]), paths, hip.from_numpy(Wflat), n)
    _record_solve("run_batch", K, S)
    assert flag == 0
    co = hip.book_get_coeffs(c.book)
    for q, (_p, _W, shift, scale, m, mom_err) in enumerate(inputs):
        R.check_solution(co[offs[q]:offs[q] + S * K], m, K, S, shift, scale, C_SOLVE, (K, S, "run_batch", R.SPREADS[q]), moment_err=mom_err)
    hip.book_set_coeffs(c.book, 0, c.coeffs)


@pytest.mark.parametrize("K,S", KS, ids=KS_IDS)
def test_device_solver_edge_branches(K, S, ctx, hip):
    """degenerate = 1: v mean(Y) / (v.v), v = [x0^k]; n = 0: zero coefficients, status 0; one distinct z with degenerate = 0
    (K > 1: G of rank 1): status 1, the book's coefficients untouched, the other jobs of a batch still written"""
    c = ctx(K, S)
    NM = (2 * K - 1) + S * K
    o0, o1, o2 = _blocks(c, 3)
    hip.book_set_coeffs(c.book, 0, c.coeffs)
    m, _, _ = R.synthetic_moments(K, S, "well")
    x0 = 1.3
    tab, st = _solve_one(hip, c, m, x0, 1.0, off0=o0, degenerate=1, x0=x0)
    v = np.array([x0 ** k for k in range(K)])
    for s in range(S):
        want = v * ((m[(2 * K - 1) + s * K] / m[0]) / (v @ v))
        assert st == 0 and np.allclose(tab[s], want, rtol=8 * K * R.EPS, atol=0.0), (K, S, s, tab[s], want)
    tab, st = _solve_one(hip, c, np.zeros(NM), 0.0, 1.0, off0=o1)
    assert st == 0 and not tab.any()
    assert not hip.book_get_coeffs(c.book)[o1:o1 + S * K].any()
    # mcx_lsm_run on zero paths: the same empty system through k3_solve
    paths = _paths(hip, c, 0)
    coeffs, status = hip.lsm_run(c.book, 0, _date(c, 0.0, 1.0, o2, -1), paths, hip.zeros(S, 1))
    _record_solve("run", K, S)
    assert status[0] == 0 and not coeffs.any()
    if K == 1:
        return
    hip.book_set_coeffs(c.book, 0, c.coeffs)
    z = np.full(200, 0.5)
    Y = np.stack([np.full(200, 1.0 + s) for s in range(S)])
    ms, _ = R.moments_ref(z, Y, K)
    tab, st = _solve_one(hip, c, ms, 0.0, 1.0, off0=o0, off1=o1)
    assert st == 1
    co = hip.book_get_coeffs(c.book)
    assert np.array_equal(co, c.coeffs), "a singular system wrote coefficients"
    got, flag = _solve_batch(hip, c, [m, ms, m], [0.0] * 3, [1.0] * 3, [o0, o1, o2])
    assert flag == 1
    co = hip.book_get_coeffs(c.book)
    assert np.array_equal(co[o1:o1 + S * K], c.coeffs[o1:o1 + S * K])
    for o in (o0, o2):
        R.check_solution(co[o:o + S * K], m, K, S, 0.0, 1.0, C_SOLVE, (K, S, "batch beside a singular job"))
    hip.book_set_coeffs(c.book, 0, c.coeffs)


# ---- C: whole runs against the oracle ---------------------------------------------------------------------------------------
def _exercise_book(kind):
    if kind == "bermudan":
        from mcx.products.swap import InterestRateSwap, IRSType
        model = cases.VasicekModel(0.0, 0.03, 0.04, 0.2, 0.012)
        und = InterestRateSwap(0.0, 3.0, 1.0, 0.035, 0.25, 0.25, IRSType.PAYER)
        prod = cases.BermudanOption(und, [float(t) for t in np.linspace(0.5, 2.5, 9)], 0.0, cases.OptionType.CALL)
        tl = np.linspace(0.0, 3.0, 9)
    elif kind == "american":
        model = cases.BlackScholesModel(0.0, 100.0, 0.04, 0.3)
        prod = cases.AmericanOption(cases.Equity("id"), 2.0, 10, 102.0, cases.OptionType.PUT)
        tl = np.linspace(0.0, 2.0, 7)
    else:
        ns, model, rm = _flexi_book(int(kind[len("flexi"):]) + 1)
        rm = cases.RiskMetrics([cases.EPEMetric(), cases.PFEMetric(0.95), cases.ENEMetric(), cases.PVMetric()],
                               exposure_timeline=rm.exposure_timeline)
        return ns, model, rm
    rm = cases.RiskMetrics([cases.EPEMetric(), cases.PFEMetric(0.95), cases.ENEMetric(), cases.PVMetric()], exposure_timeline=tl)
    return [cases.NettingSet(name="ex", products=[prod])], model, rm


def _compare_runs(kind, degree, hip, oracle, fused, mfma):
    out = {}
    for be in (hip, oracle):
        ns, model, rm = _exercise_book(kind)
        sc = cases.SimulationController(ns, model, rm, 16384, 8192, 2, cases.E, backend=be,
                                        regression_function=PolyomialRegression(degree=degree))
        if be is hip:
            sc.allow_fused = fused
            sc.use_mfma = mfma
        out[be.name] = [np.array(m, dtype=np.float64) for m in sc.run_simulation().results[0]]
        if be is hip:
            assert sc.book_plan.n_basis == degree + 1
            if fused:
                assert sc._fused is not None
                d = hip.fused_describe(sc._fused, False, True)
                assert d["kernel"] in ("lean", "fused") and not d["cva_dates"], d
    for m_i, (a, b) in enumerate(zip(out["hip"], out["oracle"])):
        assert np.allclose(a[:, 0], b[:, 0], rtol=1e-8, atol=1e-10), (kind, degree, fused, mfma, m_i, a[:, 0], b[:, 0])


RUNS = [(k, d) for k in ("bermudan", "american") for d in (0, 1, 3, 4, 5)] + \
       [(f"flexi{r}", d) for r in (4, 5, 6, 7) for d in (2, 4)]


@pytest.mark.parametrize("kind,degree", RUNS, ids=[f"{k}-deg{d}" for k, d in RUNS])
def test_exercise_products_at_other_degrees_match_oracle(kind, degree, hip, oracle):
    for fused in (True, False):
        _compare_runs(kind, degree, hip, oracle, fused, False)
    _compare_runs(kind, degree, hip, oracle, True, True)


@pytest.mark.parametrize("degree", [3, 1])
def test_cva_book_at_other_degrees_stays_off_the_cva_fast_paths(degree, hip, oracle):
    """the config-3-shaped payer-IRS CVA book: both CVA fast paths hard-code three coefficients (cva_only in mcx_fused_create,
    pure_cva in lean_date); at another degree the run takes the general date program and still matches the oracle"""
    from test_cva_date_kernel import _check, _irs_book
    out = {}
    for be in (hip, oracle):
        ns, model, rm = _irs_book(5.0, True, 0.25, 1.0)
        sc = cases.SimulationController(ns, model, rm, 70001, 4096, 2, cases.E, backend=be,
                                        regression_function=PolyomialRegression(degree=degree))
        if be is hip:
            sc.main_plan = "fused"
        out[be.name] = sc.run_simulation().results
        if be is hip:
            d = hip.fused_describe(sc._fused, False, True)
            assert d["kernel"] in ("lean", "fused") and not d["cva_dates"], d
    _check(out, ("cva", degree))


@pytest.mark.parametrize("degree", [0, 5])
def test_large_book_batched_induction_at_other_degrees(degree, hip, oracle, monkeypatch):
    """the mixed book (Americans and FlexiCalls of 2, 3 and 4 states among other products) through _perform_regression_batched /
    mcx_lsm_run_batch, against the oracle, and again with the host solver behind the batched steps.  The device run must take
    the one-call batched induction and no singular-system retry on the host solver."""
    calls = []
    run_batch = hip.lsm_run_batch

    def lsm_run_batch(book, *a, **k):
        flag = run_batch(book, *a, **k)
        calls.append((book.plan.n_basis, flag))
        return flag
    monkeypatch.setattr(hip, "lsm_run_batch", lsm_run_batch, raising=False)
    out = {}
    for be in (hip, oracle):
        ns, model, rm = cases.mixed_book_multi()
        sc = cases.SimulationController(ns, model, rm, 512, 512, 1, cases.E, backend=be,
                                        regression_function=PolyomialRegression(degree=degree))
        res = sc.run_simulation()
        out[be.name] = (np.array(res.results[0][0]), np.array(res.results[0][1]), sc)
    sc = out["hip"][2]
    states = {p.get_num_states() for p in sc.products if sc._product_requires_regression(p)}
    assert {2, 3, 4} <= states, states
    assert calls == [(degree + 1, 0)], calls
    assert getattr(sc, "lsm_singular_retries", 0) == 0
    assert np.allclose(out["hip"][0], out["oracle"][0], rtol=1e-9, atol=1e-12)
    assert np.allclose(out["hip"][1], out["oracle"][1], rtol=1e-9, atol=1e-10)
    dev = [c.numpy().copy() for c in sc.regression_coeffs]
    sc._lsm_host_solves = True
    sc._compiled_key = None
    sc.run_simulation()
    for a, b in zip(dev, [c.numpy() for c in sc.regression_coeffs]):
        assert np.allclose(a, b, rtol=1e-8, atol=1e-9 * max(np.abs(b).max(), 1e-300))


# ---- D: sensitivities -------------------------------------------------------------------------------------------------------
@pytest.fixture
def kt_recorder(hip, monkeypatch):
    """record the (K, S) of every tangent regression launch that returned"""
    lsm, lsm_step = hip.tangent_lsm, hip.tangent_lsm_step

    def tangent_lsm(book, *a, **k):
        out = lsm(book, *a, **k)
        SEEN["kt_lsm"].add(book.plan.n_basis)
        return out

    def tangent_lsm_step(book, product, *a, **k):
        out = lsm_step(book, product, *a, **k)
        SEEN["kt_lsm_step"].add((book.plan.n_basis, int(book.plan.products["n_states"][product])))
        return out
    monkeypatch.setattr(hip, "tangent_lsm", tangent_lsm, raising=False)
    monkeypatch.setattr(hip, "tangent_lsm_step", tangent_lsm_step, raising=False)
    return SEEN


def _sens_book(kind):
    if kind == "bermudan":
        ns, model, _ = _exercise_book("bermudan")
        return ns, model, cases.RiskMetrics([cases.EPEMetric(), cases.ENEMetric(), cases.PVMetric()], exposure_timeline=np.linspace(0.0, 3.0, 9))
    if kind == "irs_cva":
        return cases.irs_cva()
    ns, model, _ = _flexi_book(4, model=cases.BlackScholesModel(0, 100.0, 0.03, 0.25))      # 3 rights: S = 4
    return ns, model, cases.RiskMetrics([cases.EPEMetric(), cases.PVMetric()], exposure_timeline=np.linspace(0.0, 0.625, 6))


def _sens_controller(kind, degree, hip):
    ns, model, rm = _sens_book(kind)
    return cases.SimulationController(ns, model, rm, 8192, 8192, 2, cases.E, differentiate=True, backend=hip,
                                      regression_function=PolyomialRegression(degree=degree))


SENS = [("bermudan", 1), ("bermudan", 3), ("irs_cva", 0), ("irs_cva", 1), ("irs_cva", 3)]


@pytest.mark.parametrize("kind,degree", SENS, ids=[f"{k}-deg{d}" for k, d in SENS])
def test_forward_mode_at_other_degrees_against_replayed_bumps(kind, degree, hip, kt_recorder):
    import mcx.aad as aad
    from mcx.helpers.host_threads import single_threaded_host
    grads = {}
    for tag, h in (("tangent", None), ("fd_small", 1e-6), ("fd_default", 1e-5)):
        sc = _sens_controller(kind, degree, hip)
        if h is None:
            r = sc.run_simulation()
            passes = -(-len(sc.model.get_model_params()) // _abi.TANGENT_NP)       # TANGENT_NP parameters per pass
            assert sc.timings.get("tangent") is True and sc.timings.get("forward_mode_passes") == passes, sc.timings
        else:
            saved = aad.bump_size
            aad.bump_size = lambda theta, h=h: h * max(abs(theta), 1e-2)
            try:
                with single_threaded_host():
                    r = aad.run_with_bumps(sc)
            finally:
                aad.bump_size = saved
        grads[tag] = r.derivatives
    for ns_i in range(len(grads["tangent"])):
        for m_i in range(len(grads["tangent"][ns_i])):
            a = np.array(grads["tangent"][ns_i][m_i], dtype=np.float64)
            fds = [np.array(grads[t][ns_i][m_i], dtype=np.float64) for t in ("fd_small", "fd_default")]
            scale = max(np.abs(f).max() for f in fds) + 1e-300
            ok = np.zeros(a.shape, dtype=bool)
            for f in fds:
                ok |= np.isclose(a, f, rtol=2e-5, atol=2e-6 * scale)
            assert ok.all(), (kind, degree, m_i, a[~ok], [f[~ok] for f in fds])


FALLBACK = [("bermudan", 0), ("flexi", 1), ("bermudan", 4), ("irs_cva", 5)]


@pytest.mark.parametrize("kind,degree", FALLBACK, ids=[f"{k}-deg{d}" for k, d in FALLBACK])
def test_configurations_without_tangent_form_fall_back_to_bumps(kind, degree, hip, monkeypatch):
    """K = 1 with S > 1 and K = 2 with S = 4 have no kt_lsm_step instantiation (MCX_E_NOT_FUSABLE), K > 4 no tangent form at all
    (_NoTangentForm("basis"), raised before any tangent kernel): differentiate=True completes through run_with_bumps, the same
    numbers as calling it directly.  The 3-right FlexiCall has a tangent form at degree 2 (kt_lsm_step<3,4>)."""
    import mcx.aad as aad
    tried = []
    lsm, lsm_step = hip.tangent_lsm, hip.tangent_lsm_step

    def record(fn):
        def call(book, *a, **k):
            try:
                return fn(book, *a, **k)
            except RuntimeError as e:
                tried.append((book.plan.n_basis, str(e)))
                raise
        return call
    monkeypatch.setattr(hip, "tangent_lsm", record(lsm), raising=False)
    monkeypatch.setattr(hip, "tangent_lsm_step", record(lsm_step), raising=False)
    if kind == "flexi":
        sc = _sens_controller(kind, 2, hip)
        sc.run_simulation()
        assert sc.timings.get("tangent") is True and not tried, (sc.timings, tried)
    sc = _sens_controller(kind, degree, hip)
    r = sc.run_simulation()
    assert sc.timings.get("tangent") is False, sc.timings
    if degree + 1 <= 4:          # the library refused the (K, S) of the exercise product: MCX_E_NOT_FUSABLE (-10)
        assert tried and all(K == degree + 1 and "(-10)" in msg and "has no instantiation" in msg for K, msg in tried), tried
    else:
        assert not tried, tried
    d = aad.run_with_bumps(_sens_controller(kind, degree, hip))
    for ns_i in range(len(r.derivatives)):
        for m_i in range(len(r.derivatives[ns_i])):
            a, b = np.array(r.derivatives[ns_i][m_i], dtype=np.float64), np.array(d.derivatives[ns_i][m_i], dtype=np.float64)
            assert a.shape == b.shape and np.all(np.isfinite(a)) and np.allclose(a, b, rtol=1e-12, atol=1e-14), (kind, degree, a, b)


# ---- coverage --------------------------------------------------------------------------------------------------------------
def test_module_coverage():
    """every (K, S) of the three step kernels, every k3_solve_t specialisation and <0,0> through each of the four solve entries,
    and the tangent instantiations no other module runs: kt_lsm<1>, <2>, <4>, kt_lsm_step<2,2>, <4,2>"""
    need_step = {(v, K, S) for v in ("valu", "mfma", "batch") for K, S in KS}
    assert need_step <= SEEN["step"], sorted(need_step - SEEN["step"])
    need_solve = {(e, sp) for e in ("solve", "run", "solve_batch", "run_batch") for sp in SOLVE_SPECS | {(0, 0)}}
    assert need_solve <= SEEN["solve"], sorted(need_solve - SEEN["solve"])
    assert {1, 2, 4} <= SEEN["kt_lsm"], SEEN["kt_lsm"]
    assert {(2, 2), (4, 2)} <= SEEN["kt_lsm_step"], SEEN["kt_lsm_step"]
