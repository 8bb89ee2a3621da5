"""The book kernels (K2, csrc/k2_book.hip) route by route against the long-double interpreter of tests/book_reference.py.

mcx_eval_book launches one of nine kernels: k2_eval_book (one path per lane), the same kernel over product chunks plus
k2_sum_chunks, and seven instantiations k2_eval_book_v<PPL, FEAT>.  Every test here first asks the library which one a call will
launch (HipBackend.book_describe: the host function the launch itself uses) and asserts it; the path counts come from the
device's CU count.  The books are those of tests/book_cases.py, one per FEAT mask.

Inputs: the paths of mcx_generate_paths in a tensor with a padded leading dimension, NaN in the pad columns and in every (date,
state) row no atom names; outputs pre-filled with NaN, padded where the route allows it, with one spare exposure row.  After a
call a pad column holds the pre-fill or +0.0 and the spare row the pre-fill.

Comparison: |gpu - reference| <= TOL * M per entry (M: book_reference's magnitude of the entry) on the first 8192 paths, on a
window around every size at which the dispatch changes (all tail lanes of every size tested), and on 16,384 random paths;
mcx_resolve_atoms on the same paths; the whole matrix against the CPU oracle.  TOL_SCALAR / TOL_MULTI are four times the largest
ratio measured on the MI355X (DESIGN "The book kernels: what is pinned").  A path whose exercise margin lies within 64 TOL of its
scale is left out from that event on (at most 1e-4 of the paths); everywhere else the decisions equal the reference's.

The last test checks that the module reached every route."""
import ctypes as C

import numpy as np
import pytest
import torch

import book_cases as BC
import book_reference as R
from mcx import _abi

pytestmark = pytest.mark.gpu

BLOCK = 256
LD_PAD = 24                   # pad columns of the paths tensor and of the outputs
N_RANDOM = 16384
ORACLE_TOL = 1e-12            # whole-matrix comparison against the oracle, relative to the largest M of the row (see _check)
SEEN = set()                  # routes reached: "scalar", "chunked", (ppl, feat)
ALL_ROUTES = {"scalar", "chunked", (4, 0), (4, 1), (2, 0), (2, 1), (2, 5), (2, 7), (2, 15)}
WORST = {"scalar": 0.0, "multi": 0.0, "atoms": 0.0}


@pytest.fixture(scope="module")
def sizes(hip):
    n_cu = hip.device_info()["n_cu"]
    return {"B0": 8 * n_cu, "B1": 16 * n_cu}


def _nan(hip, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=hip.device)


class _Case:
    """one book on the GPU and on the oracle (one plan), its paths at the largest size in a padded tensor, the oracle's outputs
    on all of them and the reference on the compared paths"""

    def __init__(self, hip, oracle, name, expo_only, nmax, anchors, seed=91):
        self.hb = BC.Book(name, hip, expo_only)
        self.name, self.plan, self.book, self.nmax = name, self.hb.plan, self.hb.book, nmax
        self.obook = oracle.book_create(self.plan)
        plan, sim = self.plan, self.hb.sc._sim
        T, D = sim.plan.n_dates, sim.plan.n_state
        self.buf = _nan(hip, T, D, nmax + LD_PAD)
        hip.generate_paths(sim, seed, 0, nmax, out=self.buf[:, :, :nmax])
        R.nan_unused_rows(self.buf, self.hb.used_rows())
        hip.synchronize()
        assert torch.isnan(self.buf[:, :, nmax:]).all()
        self.cpu = self.buf[:, :, :nmax].cpu().contiguous()
        self.has_exercise = bool((plan.events["kind"] == _abi.EV_EXERCISE).any())
        self.obits = oracle.new_exercise_bits(len(plan.events), nmax)
        oracle.book_set_exercise_replay(self.obook, 1, self.obits)
        try:
            self.ocfs, self.oexpo = oracle.eval_book(self.obook, self.cpu)
        finally:
            oracle.book_set_exercise_replay(self.obook, 0, None)
        r = np.random.default_rng(seed)
        pick = [np.arange(min(8192, nmax)), r.integers(0, nmax, N_RANDOM)]
        pick += [np.arange(max(a - 4096, 0), min(a + 1024, nmax)) for a in anchors if a - 4096 < nmax]
        self.idx = np.unique(np.concatenate(pick))
        self.P = self.cpu.numpy()[:, :, self.idx]
        self._ref = {}
        self.atom_ids = np.array([k for k in range(len(plan.atoms)) if plan.atoms[k]["col"] < 0
                                  or (int(plan.atoms[k]["t_idx"]), int(plan.atoms[k]["col"])) in self.hb.used_rows()], dtype=np.int32)

    def paths(self, n):
        return self.buf[:, :, :n]

    def ref(self, tol):
        band = R.TIE_BAND * tol if self.has_exercise else 0.0
        if band not in self._ref:
            self._ref[band] = R.evaluate(self.plan, self.P, band=band)
        return self._ref[band]


_CASES = {}
BIG = {("plain", False), ("den", False), ("plain", True), ("netting", False), ("exercise", False)}      # books also run at B1 * 256 paths


@pytest.fixture(scope="module")
def case(hip, oracle, sizes):
    B0, B1 = sizes["B0"], sizes["B1"]

    def get(name, expo_only=False):
        key = (name, expo_only)
        nmax = 4099 if name == "many" else B1 * BLOCK + 1023 if key in BIG else B0 * BLOCK + 511
        if key not in _CASES:
            _CASES[key] = _Case(hip, oracle, name, expo_only, nmax, [(B0 - 1) * BLOCK, B0 * BLOCK, (B1 - 1) * BLOCK, B1 * BLOCK])
        return _CASES[key]
    yield get
    _CASES.clear()


def _route_key(d):
    return d["kernel"] if d["kernel"] != "multi" else (d["ppl"], d["feat"])


def _eval(hip, book, plan, paths, n, pad=LD_PAD):
    """mcx_eval_book straight through the library on NaN-filled outputs [NS][ld_out], [NS * E + 1][ld_out] (one spare row);
    -> (describe record, cfs [NS][n] or None, expo [NS][E][n] or None) as numpy after the checks of pad columns and spare row"""
    NS, E = plan.n_netting_sets, plan.n_expo_rows
    ld_out = n + pad
    d = hip.book_describe(book, n, ld_out)
    SEEN.add(_route_key(d))
    cfs = _nan(hip, NS, ld_out) if plan.desc.want_cfs else None
    expo = _nan(hip, NS * E + 1, ld_out) if plan.desc.want_expo else None
    hip._check(hip.lib.mcx_eval_book(hip.h, book.ptr, C.c_void_p(paths.data_ptr()), C.c_int64(n), C.c_int64(paths.stride(1)),
                                     C.c_void_p(cfs.data_ptr() if cfs is not None else 0),
                                     C.c_void_p(expo.data_ptr() if expo is not None else 0), C.c_int64(ld_out), hip._stream()),
               "mcx_eval_book")
    out = []
    for t in (cfs, expo):
        if t is None:
            out.append(None)
            continue
        a = t.cpu().numpy()
        padc = a[:-1 if t is expo else None, n:]
        assert (np.isnan(padc) | ((padc == 0.0) & ~np.signbit(padc))).all(), "a pad column holds neither the pre-fill nor +0.0"
        if t is expo:
            assert np.isnan(a[-1]).all(), "the row after the last exposure row was written"
            a = a[:-1].reshape(NS, E, ld_out)
        out.append(np.ascontiguousarray(a[..., :n]))
    return d, out[0], out[1]


def _tol(kernel):
    return R.TOL_SCALAR if kernel == "scalar" else R.TOL_MULTI


def _check(all_idx, ref, oracle_out, n, cfs, expo, kernel, tag):
    """the outputs of a call on n paths against the reference `ref` on the paths `all_idx` (those below n are compared) and
    against the oracle's outputs on all paths"""
    tol = _tol(kernel)
    sel = all_idx < n
    idx = all_idx[sel]
    worst = 0.0
    if cfs is not None:
        assert not np.isnan(cfs).any(), (tag, "cashflow entries left unwritten")
        worst = max(worst, R.worst_ratio(cfs[:, idx], ref.cfs[:, sel], ref.cfs_M[:, sel], ref.cfs_tied[:, sel]))
    if expo is not None:
        assert not np.isnan(expo).any(), (tag, "exposure entries left unwritten")
        worst = max(worst, R.worst_ratio(expo[:, :, idx], ref.expo[:, :, sel], ref.expo_M[:, :, sel], ref.expo_tied[:, :, sel]))
        for ns, row in zip(*np.nonzero(~ref.written)):          # rows nobody writes: exactly +0.0
            assert not expo[ns, row].any() and not np.signbit(expo[ns, row]).any(), (tag, ns, row)
    tied = ref.cfs_tied[:, sel].any(axis=0) | ref.expo_tied[:, :, sel].any(axis=(0, 1))
    print(f"{tag}: n={n} worst |gpu - ref| / M = {worst:.3e} (tol {tol:.3e}), tied {int(tied.sum())} of {len(idx)}")
    key = "scalar" if kernel == "scalar" else "multi"
    WORST[key] = max(WORST[key], worst)
    assert worst <= tol, (tag, n, worst, tol)
    assert tied.mean() <= 1e-4
    # The whole matrix against the oracle.  This comparison is there for what the compared paths cannot show — an entry of some
    # other path misaddressed, stale or unwritten, which is wrong by the size of a value — so its bound is loose in ulps and
    # exact in kind: 1e-12 of the largest magnitude M seen in the entry's row (two double-precision evaluations differ by
    # ~1e-15 M; a path whose exercise decision flips between them differs by a payoff and fails, as it should be looked at).
    ocfs, oexpo = oracle_out
    if cfs is not None:
        lim = ORACLE_TOL * np.asarray(ref.cfs_M.max(axis=1), dtype=np.float64)[:, None]
        assert (np.abs(cfs - ocfs.numpy()[:, :n]) <= lim).all(), (tag, "cashflows differ from the oracle's")
    if expo is not None:
        lim = ORACLE_TOL * np.asarray(ref.expo_M.max(axis=2), dtype=np.float64)[:, :, None]
        assert (np.abs(expo - oexpo.numpy()[:, :, :n]) <= lim).all(), (tag, "exposures differ from the oracle's")


def _run(hip, c, n, want_kernel, want_ppl=1, want_feat=0, tag=""):
    d, cfs, expo = _eval(hip, c.book, c.plan, c.paths(n), n)
    assert (d["kernel"], d["ppl"], d["feat"]) == (want_kernel, want_ppl, want_feat), (tag, n, d)
    assert d["n_chunks"] == 1 and d["chunk_products"] == 0
    _check(c.idx, c.ref(_tol(want_kernel)), (c.ocfs, c.oexpo), n, cfs, expo, want_kernel, f"{tag} {c.name} {_route_key(d)}")
    return d


# ---- scalar route -----------------------------------------------------------------------------------------------------------
SCALAR_BOOKS = [("plain", False), ("den", False), ("exercise", False), ("exotic", False), ("all", False), ("netting", False),
                ("plain", True), ("den", True), ("exercise", True), ("netting", True)]


@pytest.mark.parametrize("name,expo_only", SCALAR_BOOKS, ids=[f"{b}{'-expo' if e else ''}" for b, e in SCALAR_BOOKS])
def test_scalar_kernel_at_small_and_last_scalar_sizes(name, expo_only, hip, case, sizes):
    c = case(name, expo_only)
    for n in (1, 63, 257, 4099, (sizes["B0"] - 1) * BLOCK):
        _run(hip, c, n, "scalar", tag="scalar")


def test_atoms_against_the_reference(hip, case):
    """mcx_resolve_atoms (k2_resolve: dev_atom, device libm) on the compared paths of every book"""
    for name in ("plain", "den", "exercise", "exotic", "all", "netting"):
        c = case(name)
        got = hip.resolve_atoms(c.book, c.atom_ids, c.paths(c.nmax))[:, torch.from_numpy(c.idx).to(hip.device)].cpu().numpy()
        worst = max(R.worst_ratio(got[j], *R.atom(c.plan, int(k), c.P)) for j, k in enumerate(c.atom_ids))
        print(f"atoms {name}: worst |gpu - ref| / mag = {worst:.3e}")
        WORST["atoms"] = max(WORST["atoms"], worst)
        assert worst <= R.TOL_SCALAR


# ---- two paths per lane -------------------------------------------------------------------------------------------------------
TWO = [("plain", False), ("den", False), ("exercise", False), ("exotic", False), ("all", False), ("netting", False),
       ("plain", True), ("den", True), ("exercise", True), ("netting", True)]


@pytest.mark.parametrize("r", [0, 1, 256, 257, 511])
@pytest.mark.parametrize("name,expo_only", TWO, ids=[f"{b}{'-expo' if e else ''}" for b, e in TWO])
def test_two_paths_per_lane(name, expo_only, r, hip, case, sizes):
    """B0 * 256 + r: r = 0 no tail; 1: one live lane in chunk 0, chunk 1 dead; 256: chunk 1 entirely dead; 257; 511"""
    c = case(name, expo_only)
    _run(hip, c, sizes["B0"] * BLOCK + r, "multi", 2, BC.FEAT[name], tag=f"r={r}")


def test_heavier_books_stay_on_two_paths_per_lane_at_the_four_path_size(hip, case, sizes):
    """at B1 * 256 paths a book with FEAT other than 0 / DEN keeps two paths per lane; the DEN book just below B1 blocks too"""
    B1 = sizes["B1"]
    _run(hip, case("exercise"), B1 * BLOCK, "multi", 2, BC.FEAT["exercise"], tag="B1")
    c = case("den")
    assert hip.book_describe(c.book, (B1 - 1) * BLOCK + 1)["ppl"] == 4          # (the next size is the first of four paths per lane)
    _run(hip, c, (B1 - 1) * BLOCK, "multi", 2, BC.FEAT["den"], tag="B1-1")


# ---- four paths per lane ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 513, 1023])
@pytest.mark.parametrize("name,expo_only", [("plain", False), ("den", False), ("plain", True), ("netting", False)],
                         ids=["plain", "den", "plain-expo", "netting"])
def test_four_paths_per_lane(name, expo_only, r, hip, case, sizes):
    c = case(name, expo_only)
    _run(hip, c, sizes["B1"] * BLOCK + r, "multi", 4, BC.FEAT[name], tag=f"r={r}")


# ---- barrier book: scalar at every size, the oracle is the reference ---------------------------------------------------------
def test_barrier_book_stays_scalar(hip, oracle, sizes):
    hb = BC.Book("barrier", hip)
    plan, sim = hb.plan, hb.sc._sim
    obook = oracle.book_create(plan)
    for n in (1, 4099, sizes["B0"] * BLOCK, sizes["B1"] * BLOCK + 1023):
        assert hip.book_describe(hb.book, n)["kernel"] == "scalar", n
    n = 4099
    buf = _nan(hip, sim.plan.n_dates, sim.plan.n_state, n + LD_PAD)
    hip.generate_paths(sim, 5, 0, n, out=buf[:, :, :n])
    r = np.random.default_rng(3)
    inject = {}
    for p_i in (1, 2):                                   # the bridge products: two uniforms per monitored interval
        e = plan.events[int(plan.products[p_i]["ev_begin"])]
        assert e["aux"][0] == 5.0 and int(plan.coeffs[e["coeff_off"] + 1]) == p_i
        inject[p_i] = hip.from_numpy(r.uniform(0.0, 1.0, (2 * int(e["term_end"] - e["term_begin"] - 1), n)))
    hip.book_set_bridge_rng(hb.book, 1, 0, inject)
    oracle.book_set_bridge_rng(obook, 1, 0, {k: v.cpu() for k, v in inject.items()})
    d, cfs, expo = _eval(hip, hb.book, plan, buf[:, :, :n], n)
    assert d["kernel"] == "scalar" and expo is None
    ocfs, _ = oracle.eval_book(obook, buf[:, :, :n].cpu().contiguous())
    o = ocfs.numpy()
    assert (o != 0).any(axis=1).all()
    # an entry is payoff x fuzzy indicators / numeraire; an indicator clamp((. +- 0.05) / 0.1) has slope 10, so a rounding of its
    # argument (the bridge's log / exp differ between device and host libm) weighs ten times in the entry: ten times the bound
    # of the other books, relative to the row's largest entry
    assert (np.abs(cfs - o) <= 10 * ORACLE_TOL * np.abs(o).max(axis=1)[:, None]).all()


# ---- product-chunked launch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("expo_only", [False, True], ids=["many", "many-expo"])
def test_chunked_launch(expo_only, hip, case):
    c = case("many", expo_only)
    for n in (1, 257, 4099):
        d, cfs, expo = _eval(hip, c.book, c.plan, c.paths(n), n, pad=0)
        assert d["kernel"] == "chunked" and d["n_chunks"] >= 2 and d["n_chunks"] * d["chunk_products"] >= BC.N_MANY > (d["n_chunks"] - 1) * d["chunk_products"], d
        _check(c.idx, c.ref(R.TOL_SCALAR), (c.ocfs, c.oexpo), n, cfs, expo, "scalar", f"chunked many n={n}")
        # a padded output drops the chunking without notice: the scalar route, the same numbers within tolerance
        d2, cfs2, expo2 = _eval(hip, c.book, c.plan, c.paths(n), n, pad=8)
        assert d2["kernel"] == "scalar" and d2["n_chunks"] == 1, d2
        _check(c.idx, c.ref(R.TOL_SCALAR), (c.ocfs, c.oexpo), n, cfs2, expo2, "scalar", f"unchunked many n={n}")


def _integer_plan(plan, seed=2):
    """a copy of `plan` in small integers: atoms a + d x with b = 0 (numeraires: a power of two), integer weights, strikes and
    coefficients.  On integer paths every operation of the book is exact in double precision."""
    import copy
    r = np.random.default_rng(seed)
    q = copy.copy(plan)
    q.atoms, q.terms, q.events = plan.atoms.copy(), plan.terms.copy(), plan.events.copy()
    q.atoms["a"], q.atoms["d"] = r.integers(-3, 4, len(q.atoms)), r.integers(-2, 3, len(q.atoms))
    q.atoms["b"] = q.atoms["c0"] = q.atoms["c1"] = 0.0
    for k in np.unique(q.events["num_atom"]):
        q.atoms["a"][k], q.atoms["d"][k] = 2.0 ** int(r.integers(0, 3)), 0.0
    q.terms["w"] = r.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], len(q.terms))
    q.coeffs = r.integers(-3, 4, len(plan.coeffs)).astype(np.float64)
    d = _abi.BookDesc()
    for name, _t in _abi.BookDesc._fields_:
        setattr(d, name, getattr(plan.desc, name))
    d.atoms, d.terms, d.events, d.coeffs = _abi.ptr(q.atoms), _abi.ptr(q.terms), _abi.ptr(q.events), _abi.ptr(q.coeffs)
    q.desc = d
    return q


def test_chunk_images_sum_exactly_on_integer_books(hip, case):
    """integer coefficients and paths: every chunk image and their sum in chunk order are exact — bit for bit the reference"""
    c = case("many")
    q = _integer_plan(c.plan)
    book = hip.book_create(q)
    n = 4099
    r = np.random.default_rng(4)
    P = r.integers(-8, 9, (q.desc.n_dates, q.n_state, n)).astype(np.float64)
    paths = hip.from_numpy(P)
    d, cfs, expo = _eval(hip, book, q, paths, n, pad=0)
    assert d["kernel"] == "chunked" and d["n_chunks"] >= 2
    ref = R.evaluate(q, P)
    assert np.array_equal(cfs, np.asarray(ref.cfs, dtype=np.float64)) and np.array_equal(ref.cfs, cfs.astype(R.LD))
    assert np.array_equal(expo, np.asarray(ref.expo, dtype=np.float64)) and np.array_equal(ref.expo, expo.astype(R.LD))
    assert (ref.cfs != 0).any() and (ref.expo != 0).any(axis=2).all()
    d2, cfs2, expo2 = _eval(hip, book, q, paths, n, pad=8)          # the same book through the scalar route
    assert d2["kernel"] == "scalar" and np.array_equal(cfs2, cfs) and np.array_equal(expo2, expo)


# ---- exercise record and replay -------------------------------------------------------------------------------------------------
def _bits(hip, c, n):
    return torch.zeros((len(c.plan.events), n + LD_PAD), dtype=torch.uint8, device=hip.device)


@pytest.mark.parametrize("route", ["scalar", "multi"])
def test_exercise_record(route, hip, case, sizes):
    """record: the bits equal the reference's decisions outside the tie band (and the outputs are those of a plain run)"""
    c = case("exercise")
    n = 4099 if route == "scalar" else sizes["B0"] * BLOCK + 257
    tol = R.TOL_SCALAR if route == "scalar" else R.TOL_MULTI
    bits = _bits(hip, c, n)
    hip.book_set_exercise_replay(c.book, 1, bits)
    try:
        d, cfs, expo = _eval(hip, c.book, c.plan, c.paths(n), n)
    finally:
        hip.book_set_exercise_replay(c.book, 0, None)
    assert (d["kernel"], d["ppl"], d["feat"]) == ((route, 1, 0) if route == "scalar" else ("multi", 2, BC.FEAT["exercise"]))
    _check(c.idx, c.ref(tol), (c.ocfs, c.oexpo), n, cfs, expo, route, f"record {route}")
    got = bits.cpu().numpy()
    assert not got[:, n:].any(), "a byte beyond the path count was written"
    ref = c.ref(tol)
    sel = c.idx < n
    idx = c.idx[sel]
    n_dec = 0
    for pr in c.plan.products:
        seen_tie = np.zeros(len(idx), dtype=bool)
        for q in range(int(pr["ev_begin"]), int(pr["ev_end"])):
            if q in ref.decisions:
                seen_tie |= ref.tie_at[q][sel]
                assert np.array_equal((got[q, idx] & 1).astype(bool)[~seen_tie], ref.decisions[q][sel][~seen_tie]), (route, q)
                n_dec += int(ref.decisions[q][sel].sum())
    assert n_dec > 0


@pytest.mark.parametrize("route", ["scalar", "multi"])
def test_exercise_replay(route, hip, oracle, case, sizes):
    """replay of random bits with the coefficients perturbed again: cashflows, exposures and states follow the bits exactly as
    the reference does replaying the same bits — compared at TOL with no tie allowance (replay has no indicator)"""
    c = case("exercise")
    n = 4099 if route == "scalar" else sizes["B0"] * BLOCK + 257
    r = np.random.default_rng(12)
    hbits = r.integers(0, 2, (len(c.plan.events), n + LD_PAD), dtype=np.uint8)
    bits = torch.from_numpy(hbits).to(hip.device)
    first = c.plan.coeffs.copy()
    try:
        c.hb.set_coeffs(hip, BC.perturbed_coeffs(c.hb.sc, c.hb.base_coeffs, seed=BC.COEFF_SEED + 1))
        hip.book_set_exercise_replay(c.book, 2, bits)
        d, cfs, expo = _eval(hip, c.book, c.plan, c.paths(n), n)
        sel = c.idx < n
        ref = R.evaluate(c.plan, c.P[:, :, sel], replay={q: hbits[q, c.idx[sel]].astype(bool) for q in range(len(c.plan.events))})
        obits = torch.from_numpy(np.ascontiguousarray(hbits[:, :n]))
        oracle.book_set_exercise_replay(c.obook, 2, obits)
        oout = oracle.eval_book(c.obook, c.cpu[:, :, :n].contiguous())
    finally:
        hip.book_set_exercise_replay(c.book, 0, None)
        oracle.book_set_exercise_replay(c.obook, 0, None)
        c.hb.set_coeffs(hip, first)
    assert (d["kernel"], d["ppl"], d["feat"]) == ((route, 1, 0) if route == "scalar" else ("multi", 2, BC.FEAT["exercise"]))
    assert torch.equal(bits.cpu(), torch.from_numpy(hbits)), "replay wrote the bits"
    assert not ref.cfs_tied.any() and not ref.expo_tied.any()
    _check(c.idx[sel], ref, oout, n, cfs, expo, route, f"replay {route}")
    # states: the exposure of a date is the polynomial of the state the bits led to — a wrong state shows as a wrong row above;
    # the replayed decisions took both branches in every state
    fs = ref.final_state[1]
    assert len(np.unique(fs)) == 4


# ---- value polynomials on the multi-path route ----------------------------------------------------------------------------------
def test_value_polynomial_on_the_multi_path_route(hip, oracle, sizes):
    """a bond option whose underlying has >= 6 terms, the path columns ordered by the polynomial's x: whole waves inside the verified
    range, whole waves outside, mixed waves at the two boundaries (the __all(in) fall-back).  Collapsed: within the reference
    tolerance plus the project's 1e-11 relative of the polynomial; bit-equal to the uncollapsed run on every wave wholly outside."""
    model = BC._vasicek()
    und = BC.cases.Bond(0.0, 4.0, 1.0, 0.5, True, 0.04, "r")
    opt = BC._named(BC.cases.EuropeanOption(und, 0.5, 0.95, BC.cases.OptionType.CALL, asset_id="r"), "bond_call")
    rm = BC.cases.RiskMetrics([BC.cases.PVMetric()])
    sc = BC.cases.SimulationController([BC.cases.NettingSet(name="o", products=[opt])], model, rm, 1024, 0, 2, BC.cases.A, backend=hip)
    sc.allow_fused = False
    sc.prepare()
    plan, book, sim = sc.book_plan, sc.book, sc._sim
    ev = int(plan.products[0]["ev_begin"])
    assert plan.products[0]["ev_end"] - ev == 1 and plan.events[ev]["term_end"] - plan.events[ev]["term_begin"] >= 6
    n = sizes["B0"] * BLOCK + 257
    ta = plan.atoms[plan.terms[plan.events[ev]["term_begin"]:plan.events[ev]["term_end"]]["atom"]]
    assert len(set(zip(ta["t_idx"].tolist(), ta["col"].tolist()))) == 1          # one state variable of one date: the polynomial's x
    t_idx, col = int(ta["t_idx"][0]), int(ta["col"][0])
    raw = hip.generate_paths(sim, 17, 0, n)
    order = torch.argsort(raw[t_idx, col])
    buf = _nan(hip, sim.plan.n_dates, sim.plan.n_state, n + LD_PAD)
    buf[:, :, :n] = raw[:, :, order]
    x = buf[t_idx, col, :n].cpu().numpy()
    lo_i, hi_i = n // 4 + 19, 3 * n // 4 + 37              # inside a wave each: the waves at the two boundaries are mixed
    lo, hi = float(x[lo_i]), float(x[hi_i])
    d0, cfs0, _ = _eval(hip, book, plan, buf[:, :, :n], n)
    assert (d0["kernel"], d0["ppl"], d0["feat"]) == ("multi", 2, 0)
    T, D = sim.plan.n_dates, sim.plan.n_state
    los, his = np.full((T, D), lo), np.full((T, D), hi)
    assert hip.book_collapse_values(book, los, his, pad=0.0, rel_tol=1e-14, min_terms=6) >= 1
    try:
        d1, cfs1, _ = _eval(hip, book, plan, buf[:, :, :n], n)
    finally:
        hip.book_collapse_values(book, None, None)
    assert d1 == d0
    inside = (x >= lo) & (x <= hi)
    blk = np.arange(n) // (2 * BLOCK)          # a block carries 2 * 256 consecutive paths: lane t has paths t and 256 + t of them
    w64 = (np.arange(n) % BLOCK) // 64
    grp = blk * 4 + w64                          # the paths of one wave: both chunks of its 64 lanes
    has_in = np.zeros(grp.max() + 1, dtype=bool)
    np.logical_or.at(has_in, grp, inside)
    all_in = np.ones(grp.max() + 1, dtype=bool)
    np.logical_and.at(all_in, grp, inside)
    outside_wave, inside_wave = ~has_in[grp], all_in[grp]
    assert outside_wave.sum() > 10000 and inside_wave.sum() > 10000 and (~outside_wave & ~inside_wave).sum() >= 128
    assert np.array_equal(cfs1[:, outside_wave], cfs0[:, outside_wave]), "a wave wholly outside the range took the polynomial"
    assert np.array_equal(cfs1[:, ~inside_wave], cfs0[:, ~inside_wave]), "a mixed wave took the polynomial"
    assert (cfs1[:, inside_wave] != cfs0[:, inside_wave]).any(), "no wave took the polynomial"
    r = np.random.default_rng(8)
    idx = np.unique(np.concatenate([np.arange(lo_i - 2048, lo_i + 2048), np.arange(hi_i - 2048, hi_i + 2048), r.integers(0, n, 8192),
                                    np.arange(n - 2048, n)]))
    P = buf[:, :, :n].cpu().numpy()[:, :, idx]
    ref = R.evaluate(plan, P)
    err = np.abs(cfs1[:, idx].astype(R.LD) - ref.cfs)
    bound = (R.TOL_MULTI + 1e-11) * ref.cfs_M
    print(f"vpoly: worst collapsed ratio {float((err / ref.cfs_M).max()):.3e}, uncollapsed "
          f"{R.worst_ratio(cfs0[:, idx], ref.cfs, ref.cfs_M):.3e}")
    assert (err <= bound).all()
    assert R.worst_ratio(cfs0[:, idx], ref.cfs, ref.cfs_M) <= R.TOL_MULTI


# ---- coverage -------------------------------------------------------------------------------------------------------------------
def test_every_route_was_reached():
    print(f"worst ratios: scalar {WORST['scalar']:.3e}, multi-path {WORST['multi']:.3e}, atoms {WORST['atoms']:.3e}")
    assert SEEN == ALL_ROUTES, (ALL_ROUTES - SEEN, SEEN - ALL_ROUTES)
