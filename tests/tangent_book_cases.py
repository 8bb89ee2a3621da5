"""Inputs of the dual book kernel tests (tests/test_tangent_book_reference.py, tests/test_tangent_book_kernels.py), all made on the host.

Books: those of tests/book_cases.py without exotic events — plain, den, netting (two netting sets, the empty product, the threshold),
exercise (a FlexiCall with 3 rights and a Bermudan) — and
  flexis     FlexiCalls with 1 and 2 rights: with `exercise`, n_states takes 2, 3 and 4
  bs_expo    the call and the put of book_cases.all_ (analytic Black-Scholes exposures, one event at tau == 0) with the exercise
             products and NO exotic event: the unarmed instantiation of kt_eval runs
  mixed_cva  cases.mixed_cva: survival atoms with b != 0
each compiled on the CPU oracle backend at regression degree K - 1 (n_basis = K in 2, 3, 4), coefficients perturbed as in
book_cases.  The GPU tests create their device book from the SAME plan, so what the host test establishes about these inputs (no
path near a kink or an exercise tie, every exercise state populated) holds for the GPU run.

Paths come from the oracle's path generator; dpaths, datoms and dcoeffs are random, scaled to what they differentiate, and rounded
to 16 bits below the binade of that number: x +- 2^-20 dx is then exact in float64 and a central difference of the float64 inputs
is a difference along exactly this direction.  Rows of the paths no atom names hold NaN."""
import numpy as np

import book_cases as BC
import book_reference as R
import cases
import tangent_book_reference as T
from mcx import _abi

NP = _abi.TANGENT_NP
SIZES = [1, 255, 257]
BLOCK = 256
N_CU_MI355X = 256             # the host test checks the grid-stride sets of this device; the GPU test takes the device's own count
CAP_PROFILES, CAP_PICK = 64, 256          # block caps of mcx_tangent_profiles / mcx_tangent_pick (csrc/kt_book.hip)
SEED = 2024


def ld_of(n):
    return (n + 63) // 64 * 64 + 64


def stride_size(cap_blocks):
    """just past the first grid-stride round of a kernel whose grid is mcx_grid_for(n, 256, cap_blocks)"""
    return cap_blocks * BLOCK + 257


def lsm_step_cap(n_cu):
    return 2 * n_cu


def quantize(d, x):
    """d rounded to a multiple of 2^(e - 16), e the binade of x (x == 0: of d itself)"""
    d, x = np.asarray(d, dtype=np.float64), np.broadcast_to(np.asarray(x, dtype=np.float64), np.shape(d))
    ref = np.where(x != 0.0, np.abs(x), np.abs(d))
    ok = np.isfinite(ref) & (ref > 0)
    q = np.ones_like(d)
    q[ok] = 2.0 ** (np.floor(np.log2(ref[ok])) - 16)
    return np.where(ok, np.round(d / q) * q, d)


def flexis(expo_only=False):
    ids, model = BC._eq_rates_model(1)
    a = ids[0]
    o1 = [cases.EuropeanOption(cases.Equity(a), 0.2 * (k + 1), 98.0 + 1.0 * k, cases.OptionType.PUT, asset_id=a) for k in range(5)]
    o2 = [cases.EuropeanOption(cases.Equity(a), 0.2 * (k + 1), 96.5 + 1.5 * k, cases.OptionType.PUT, asset_id=a) for k in range(5)]
    P = [BC._named(cases.FlexiCall(o1, 1, asset_id=a), "flexi1"), BC._named(cases.FlexiCall(o2, 2, asset_id=a), "flexi2")]
    return [cases.NettingSet(name="ns", products=P)], model, BC._metrics(expo_only, BC._TL_EQ), 1, cases.E


def bs_expo(expo_only=False):
    ids = ["eq0", "eq1"]
    model = cases.BlackScholesMulti(0.0, 0.03, ids, [100.0, 105.0], [0.25, 0.22], np.array([[1.0, 0.3], [0.3, 1.0]]))
    P = ([BC._named(cases.EuropeanOption(cases.Equity(ids[0]), 0.8, 95.0, cases.OptionType.CALL, asset_id=ids[0]), "call"),
          BC._named(cases.EuropeanOption(cases.Equity(ids[1]), 1.0, 110.0, cases.OptionType.PUT, asset_id=ids[1]), "put")]
         + BC._exercise_products(ids[0]))
    return [cases.NettingSet(name="ns", products=P)], model, BC._metrics(expo_only, BC._TL_EQ, pfe=True), 1, cases.A


def _mixed_cva(expo_only=False):
    ns, model, rm = cases.mixed_cva()
    return ns, model, rm, 2, cases.E


BUILDERS = {"plain": BC.plain, "den": BC.den, "netting": BC.netting, "exercise": BC.exercise, "flexis": flexis, "bs_expo": bs_expo,
            "mixed_cva": _mixed_cva}
# (book, n_basis) pairs of mcx_tangent_eval; `exercise` at all three basis sizes
EVAL_BOOKS = [("plain", 3), ("den", 3), ("netting", 3), ("exercise", 2), ("exercise", 3), ("exercise", 4), ("flexis", 2), ("flexis", 3),
              ("bs_expo", 3)]
# the nine instantiations kt_lsm_step<K, S>: (K, S) -> (book, product name)
LSM_STEP = {(2, 1): ("den", "swap_uneq"), (3, 1): ("den", "swap_uneq"), (4, 1): ("den", "swap_uneq"),
            (2, 2): ("flexis", "flexi1"), (3, 2): ("exercise", "bermudan"), (4, 2): ("exercise", "bermudan"),
            (2, 3): ("flexis", "flexi2"), (3, 3): ("flexis", "flexi2"), (3, 4): ("exercise", "flexi")}
EVAL_IDS = [f"{b}-K{k}" for b, k in EVAL_BOOKS]
COEFF_SEEDS = {("exercise", 4): 6}              # (book, K) -> seed of perturbed_coeffs where book_cases.COEFF_SEED leaves an exercise state empty


class Book:
    """one book compiled on `backend` (the CPU oracle) at n_basis = K with perturbed coefficients"""

    def __init__(self, name, K, backend):
        ns, model, rm, steps, scheme = BUILDERS[name]()
        sc = cases.SimulationController(ns, model, rm, 1024, BC.N_PRE, steps, scheme, backend=backend,
                                        regression_function=cases.PolyomialRegression(degree=K - 1))
        sc.allow_fused = False
        sc.prepare()
        self.name, self.K, self.sc = name, K, sc
        assert sc.book_plan.n_basis == K
        backend.book_set_coeffs(sc.book, 0, BC.perturbed_coeffs(sc, sc.book_plan.coeffs.copy(), seed=COEFF_SEEDS.get((name, K), BC.COEFF_SEED)))
        self.plan = BC.with_empty_product(sc.book_plan, 0, 1) if name == "netting" else sc.book_plan
        self.shift = 1 if name == "netting" else 0                  # products after the first moved by the spliced one
        ev = self.plan.events
        assert not ((ev["kind"] == _abi.EV_OPTION) & (ev["aux"][:, 0] != 0.0)).any()
        self.ev_param = None
        bs = np.nonzero(ev["kind"] == _abi.EV_EXPO_BS)[0]
        if len(bs):
            self.ev_param = np.full((len(ev), 2), -1, dtype=np.int32)
            for k, q in enumerate(bs):                               # every slot and "none" occur for sigma and for rate
                self.ev_param[q] = (k % (NP + 1) - 1, (k + 2) % (NP + 1) - 1)

    def used_rows(self):
        a = self.plan.atoms
        return {(int(t), int(c)) for t, c in zip(a["t_idx"], a["col"]) if c >= 0}

    def product(self, pname):
        """index of the named product in the plan"""
        p_i = [p.name for p in self.sc.products].index(pname)
        return p_i + (self.shift if p_i > 0 else 0)

    def lsm_steps(self, pname):
        """the first two entries of the product's backward regression schedule that roll a window:
        [(roll_begin, roll_end, numeraire atom, explanatory atom)]"""
        p_i = [p.name for p in self.sc.products].index(pname)
        jobs, _ = self.sc._regression_plan()
        _, _, sched, atoms = next(j for j in jobs if j[0] == p_i)
        out = [(int(e[1]), int(e[2]), int(a[0]), int(a[1])) for e, a in zip(sched, atoms) if e[2] > e[1]]
        assert len(out) >= 2
        return out[:2]


_BOOKS = {}


def book(name, K, backend):
    if (name, K) not in _BOOKS:
        _BOOKS[name, K] = Book(name, K, backend)
    return _BOOKS[name, K]


class Inputs:
    """paths [T][D][n], dpaths [NP][T][D][n], datoms [n_atoms][5][NP], coeffs [n_coeffs], dcoeffs [n_coeffs][NP] of one book at n paths"""


def inputs(b, n, backend, seed=SEED):
    plan = b.plan
    x = Inputs()
    x.n, x.seed = n, seed
    rng = np.random.default_rng([seed, n, b.K])
    paths = backend.generate_paths(b.sc._sim, seed + n, 0, n).numpy().copy()
    dpaths = quantize(rng.normal(0.0, 1.0, (NP,) + paths.shape) * np.abs(paths)[None] * 0.01, paths[None])
    used = b.used_rows()
    R.nan_unused_rows(paths, used)
    for q in range(NP):
        R.nan_unused_rows(dpaths[q], used)
    x.paths, x.dpaths = paths, dpaths
    datoms = rng.normal(0.0, 0.3, (len(plan.atoms), 5, NP))
    datoms[:, 3:] *= 0.1
    datoms[plan.atoms["b"] == 0.0, 2:] = 0.0                         # no exponential part: nothing to differentiate
    fields = np.stack([plan.atoms[f] for f in ("a", "d", "b", "c0", "c1")], axis=1)
    x.datoms = quantize(datoms, fields[:, :, None])
    x.coeffs = plan.coeffs.copy()
    c = np.abs(x.coeffs)[:, None]
    x.dcoeffs = quantize(rng.normal(0.0, 0.1, (len(x.coeffs), NP)) * np.where(c > 0, c, 0.1), x.coeffs[:, None])
    return x


def padded(a, ld, fill=np.nan):
    out = np.full(a.shape[:-1] + (ld,), fill)
    out[..., :a.shape[-1]] = a
    return out


def centering(plan, x_atom, paths):
    """(shift, scale) of the explanatory variable on these paths: z = (x - shift) scale in [-1, 1]"""
    v = np.asarray(R.atom(plan, x_atom, paths)[0], dtype=np.float64)
    lo, hi = float(v.min()), float(v.max())
    return 0.5 * (lo + hi), (2.0 / (hi - lo) if hi > lo else 1.0)


# ---- what the host test and the GPU tests ask of a case, from the restatement alone ----------------------------------------------------
def eval_case(b, x):
    """(yardstick, bound, long-double run, its DualBook) of mcx_tangent_eval on these inputs.  The yardstick is floored by the longest
    event of the main pass, 2^-52 (terms + 4); the run carries the longest event of every row (cfs_terms, expo_terms) for row_bounds"""
    run = {}
    for dt in (np.float64, T.LD):
        db = T.DualBook(b.plan, x.paths, x.dpaths, x.datoms, dtype=dt)
        run[dt] = db.evaluate(x.coeffs, x.dcoeffs, b.ev_param)
    lo, hi = run[np.float64], run[T.LD]
    y = max(T.yardstick(lo.cfs, hi.cfs, hi.cfs_terms), T.yardstick(lo.expo, hi.expo, hi.expo_terms))
    for q in hi.decisions:
        assert np.array_equal(hi.decisions[q], lo.decisions[q]), q
    return y, T.FACTOR * y, hi, db


def lsm_step_ref(b, x, p_i, step, W, dW):
    """one step (roll_begin, roll_end, numeraire atom, explanatory atom) of product p_i on the float64 cache (W, dW), in float64 and in
    long double: -> (the entry point's arguments, (W', dW', summands) in long double, yardstick of W' / dW', yardstick of the summands),
    both floored by the longest event of the rolled window; asserts that no path is within 64 bounds of a kink or a tie"""
    r0, r1, num_atom, x_atom = step
    shift, scale = centering(b.plan, x_atom, x.paths)
    res = {}
    for dt in (np.float64, T.LD):
        db = T.DualBook(b.plan, x.paths, x.dpaths, x.datoms, dtype=dt)
        res[dt] = db.lsm_step(p_i, r0, r1, num_atom, x_atom, shift, scale, W, dW, x.coeffs, terms=True)
    cf = int(b.plan.products[p_i]["cf_begin"])
    longest = db.longest(cf + r0, cf + r1)
    lo, hi = res[np.float64], res[T.LD]
    y_w = max(T.yardstick(lo[0], hi[0], longest), T.yardstick(lo[1], hi[1], longest))
    y_t = T.yardstick(lo[2], hi[2], longest)
    assert db.smallest_margin() > T.TIE_FACTOR * T.FACTOR * y_w, (step, db.smallest_margin(), y_w)
    return (p_i, r0, r1, num_atom, x_atom, shift, scale), hi, y_w, y_t


# ---- fabricated exposures for the metric kernels ---------------------------------------------------------------------------------
H = 0.375                     # the threshold of the fabricated exposures
EDGES = [H, -H, np.nextafter(H, np.inf), np.nextafter(-H, -np.inf), np.nextafter(H, 0.0), 0.0, -0.0]


MODES = ("thresholded", "unthresholded", "collateralised")
ROWS = np.array([0, 1, 2, 3, 1], dtype=np.int32)          # exposure row of every metric date of the fabricated exposures


def metric_mode(mode, rows):
    """(threshold, collateralised, delayed rows) of an unsecured mode; the delayed rows hold -1 and a repeated row"""
    if mode == "unthresholded":
        return 0.0, False, None
    if mode == "thresholded":
        return H, False, None
    delayed = np.array([-1] + [int(rows[max(m - 2, 0)]) for m in range(1, len(rows))], dtype=np.int32)
    assert (delayed == -1).any() and (len(rows) < 3 or delayed[1] == delayed[2])
    return H, True, delayed


def fabricated_expo(n, n_rows=4, seed=5):
    """expo [1+NP][n_rows][n]: values around +-H with the exact edges planted (as far as n allows), tangents random and non-zero"""
    rng = np.random.default_rng([seed, n])
    e = np.empty((1 + NP, n_rows, n))
    e[0] = rng.normal(0.0, 1.0, (n_rows, n)) * H * 1.5
    e[1:] = rng.normal(0.0, 1.0, (NP, n_rows, n)) + 3.0
    for r in range(n_rows):
        at = rng.permutation(n)[:len(EDGES)]
        for k, i in enumerate(at):
            e[0, r, i] = EDGES[(k + r) % len(EDGES)]
    return e
