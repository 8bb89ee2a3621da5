"""k4_fva (csrc/k4_fva.hip) through the C ABI, mcx_reduce_fva: per-path integrands and reduced records against the numpy restatement
of the table (tests/fva_reference.py), the bit-for-bit identities of the operation order, the grid stride, every refusal.

Inputs as in tests/test_xva_kernels.py: small compiled controllers (payer swap under ModelConfig[Vasicek, CIR++(cp), CIR++(own)],
all three correlated, tests/xva_cases.py) give the exposure block, the paths, the book and its atoms.  They are re-placed in tensors
with a padded leading dimension and NaN beyond the n paths of a case.  The restatement is fed the unsecured exposures
(tests/metric_reference.unsecured_np) and the two survival atom arrays as mcx_resolve_atoms gives them on the device — the same
dev_atom the kernel inlines, tied here to the oracle's atoms at 1e-13 — so what is compared is the table's arithmetic and the
reduction, not two exponentials.  The weight tables come from two different dict curves through the engine's funding_weights
(pinned on the CPU in tests/test_fva_host.py); one variant has a lending table of exact zeros, one a negative borrowing table.

Bounds.  Per path: the yardstick of a case is the restatement's own float64-against-long-double gap over the case's largest
integrand; the device must sit within max(4 x yardstick, E x 2.2e-16) of the long-double restatement.  Records: mean at rtol 1e-12,
error at rtol 1e-9.  The test prints each case's figures before it asserts; the figures measured on the MI355X are in README
"Funding valuation adjustment".

One launch shape (grid-stride above 8 blocks per CU), so there is no second kernel to test; the grid-stride case runs one block more
than the cap holds, plus a partial one."""
import ctypes as C

import numpy as np
import pytest

import fva_reference as fr
import metric_reference as mr
import xva_cases as xc
from mcx import _abi
from mcx.metrics.fva_metric import FVAMetric, funding_weights
from mcx.metrics.metric import combine_acc, mean_and_error
from mcx.plan import UnsecuredSpec

pytestmark = pytest.mark.gpu

TIMELINES = {1: np.array([0.5]), 2: np.array([0.5, 1.0]), 11: xc.TIMELINE}
N_MAX, COUNTS, PAD = 513, (1, 255, 257, 513), 7
KINDS = ("plain", "threshold", "mpor")
NAMES = {"both": (True, True), "own": (False, True), "cp": (True, False), "none": (False, False)}


def place(be, mat, n):
    """mat [..][>= n] -> device view [..][n] of a NaN-filled buffer with leading dimension n + PAD"""
    lead, ld = mat.shape[:-1], n + PAD
    buf = np.full(lead + (ld,), np.nan)
    buf[..., :n] = mat[..., :n]
    return be.from_numpy(buf)[..., :n]


def weight_tables(tl):
    """variant -> (borrowing, lending) tables of E-1 weights"""
    nd = len(tl) - 1
    curves = (np.array(funding_weights(fr.BORROW_CURVE, tl)), np.array(funding_weights(fr.LEND_CURVE, tl)))
    return {"curves": curves, "zero lend": (curves[0], np.zeros(nd)),
            "negative": (np.array(funding_weights({1.0: -0.02, 2.0: -0.01}, tl)), curves[1]), "unit": (np.ones(nd), np.ones(nd))}


@pytest.fixture(scope="module")
def setups(hip, oracle):
    """E -> the compiled controller's book, atoms, exposure block and paths (numpy), the three descriptors, the weight tables"""
    out = {}
    for E, tl in TIMELINES.items():
        sc = xc.controller(hip, [FVAMetric(fr.BORROW_CURVE, fr.LEND_CURVE, counterparty_id="cp", own_id="own")], n_main=N_MAX, n_pre=1024,
                           timeline=tl, threshold=xc.THRESHOLD, mpor=xc.MPOR)
        sc.run_simulation()
        cp, own = sc._fva_atoms[0]
        assert len(cp) == len(own) == E - 1
        paths, expo = sc.last_state["paths"], sc.last_state["expo"][0]
        ids = list(cp) + list(own)
        if ids:
            at = hip.resolve_atoms(sc.book, ids, paths.contiguous()).cpu().numpy().reshape(2, E - 1, N_MAX)
            at_o = oracle.resolve_atoms(sc.book, ids, paths.cpu().contiguous()).numpy().reshape(2, E - 1, N_MAX)
            assert np.allclose(at, at_o, rtol=1e-13, atol=0.0)
        else:
            at = np.zeros((2, 0, N_MAX))
        rows, delayed = sc.metric_exposure_indices.numpy(), sc.netting_set_delayed_exposure_indices[0].numpy()
        out[E] = dict(sc=sc, book=sc.book, cp=cp, own=own, atoms=at, paths=paths.cpu().numpy(), expo=expo.cpu().numpy(),
                      weights=weight_tables(tl),
                      desc={"plain": (rows, None, 0.0, False), "threshold": (rows, None, xc.THRESHOLD, False),
                            "mpor": (rows, delayed, xc.THRESHOLD, True)})
        for wb, wl in out[E]["weights"].values():
            assert len(wb) == len(wl) == E - 1
    w = out[11]["weights"]
    assert not np.array_equal(*w["curves"]) and np.all(w["curves"][0] > 0) and np.all(w["curves"][1] > 0)
    assert not w["zero lend"][1].any() and np.all(w["negative"][0] < 0)
    return out


def reference(s, kind, n, names="both", weights="curves", negate=False, dtype=np.longdouble):
    cp, own = NAMES[names]
    x = mr.unsecured_np(-s["expo"] if negate else s["expo"], *s["desc"][kind])[:, :n]
    a = s["atoms"][:, :, :n]
    wb, wl = s["weights"][weights]
    return x, fr.integrands(x, a[0] if cp else None, a[1] if own else None, wb, wl, dtype=dtype)


def call(hip, s, kind, n, names="both", weights="curves", negate=False, swap_names=False, swap_weights=False):
    """records [3] of the first n paths"""
    expo = place(hip, -s["expo"] if negate else s["expo"], n)
    paths = place(hip, s["paths"], n)
    cp, own = NAMES[names]
    a, b = s["cp"] if cp else None, s["own"] if own else None
    if swap_names:
        a, b = b, a
    wb, wl = s["weights"][weights]
    if swap_weights:
        wb, wl = wl, wb
    return hip.reduce_fva(s["book"], UnsecuredSpec(*s["desc"][kind]), a, b, wb, wl, expo, paths)


def stats(rec):
    return np.array([mean_and_error(np.array([r["n"], r["shift"], r["s1"], r["s2"]])) for r in rec])


def one_path_calls(hip, s, kind, names, weights):
    """[3][N_MAX] device integrands: the shift of the record of a one-path call"""
    expo, paths = place(hip, s["expo"], N_MAX), place(hip, s["paths"], N_MAX)
    cp, own = NAMES[names]
    a, b = s["cp"] if cp else None, s["own"] if own else None
    wb, wl = s["weights"][weights]
    v = np.zeros((3, N_MAX))
    u = UnsecuredSpec(*s["desc"][kind])
    for i in range(N_MAX):
        rec = hip.reduce_fva(s["book"], u, a, b, wb, wl, expo[:, i:i + 1], paths[:, :, i:i + 1])
        assert np.all(rec["n"] == 1.0) and np.all(rec["s1"] == 0.0) and np.all(rec["s2"] == 0.0)
        v[:, i] = rec["shift"]
    return v


@pytest.fixture(scope="module")
def per_path(hip, setups):
    """(E, kind) -> [3][N_MAX] device integrands with both names and the two curves' weights"""
    return {(E, kind): one_path_calls(hip, s, kind, "both", "curves") for E, s in setups.items() for kind in KINDS}


@pytest.mark.parametrize("E", sorted(TIMELINES))
def test_inputs_take_both_signs(E, setups):
    """at least a quarter of the (path, date) cells positive and a quarter negative, for every descriptor and path count > 1"""
    for kind in KINDS:
        for n in COUNTS:
            x, _ = reference(setups[E], kind, n)
            pos, neg = (x > 0).mean(), (x < 0).mean()
            print(f"E={E} {kind} n={n}: positive {pos:.3f} negative {neg:.3f}")
            if n > 1:
                assert pos >= 0.25 and neg >= 0.25, (E, kind, n, pos, neg)


def check_records(rec, ld, n, tag):
    got = stats(rec)
    m_ref, e_ref = (np.asarray(t, dtype=np.float64) for t in fr.mean_and_error(ld))
    print(f"{tag}: mean off {np.abs(got[:, 0] - m_ref).max():.3e}, error off {0.0 if n == 1 else np.abs(got[:, 1] - e_ref).max():.3e}")
    assert np.all(rec["n"] == float(n))
    assert np.allclose(got[:, 0], m_ref, rtol=1e-12, atol=0.0), (tag, got[:, 0], m_ref)
    assert np.allclose(got[:, 1], e_ref, rtol=1e-9, atol=0.0, equal_nan=True), (tag, got[:, 1], e_ref)
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("E", sorted(TIMELINES))
def test_integrands_and_records_against_the_restatement(E, kind, hip, setups, per_path):
    s, floor = setups[E], E * 2.2e-16
    worst = [0.0, 0.0]
    for n in COUNTS:
        _, ld = reference(s, kind, n)
        _, f64 = reference(s, kind, n, dtype=np.float64)
        scale = float(np.abs(ld).max())
        dev = per_path[E, kind][:, :n]
        if E == 1:
            assert scale == 0.0 and not dev.any()
            yard = gap = 0.0
        else:
            assert scale > 0.0
            yard = float(np.abs(f64.astype(np.longdouble) - ld).max()) / scale
            gap = float(np.abs(dev.astype(np.longdouble) - ld).max()) / scale
        worst = [max(worst[0], yard), max(worst[1], gap)]
        print(f"E={E} {kind} n={n}: yardstick {yard:.3e}, per-path gap {gap:.3e}, bound {max(4.0 * yard, floor):.3e}")
        assert gap <= max(4.0 * yard, floor), (E, kind, n, gap, yard)
        rec = call(hip, s, kind, n)
        assert np.array_equal(rec["shift"], dev[:, 0])
        got = check_records(rec, ld, n, f"E={E} {kind} n={n} both")
        if E == 1 and n > 1:
            assert not got.any()                                              # exactly (0, 0), three times
        # the other name choices and weight tables: records
        for names, weights in (("own", "curves"), ("cp", "curves"), ("none", "curves"), ("both", "zero lend"), ("both", "negative")):
            _, ld_v = reference(s, kind, n, names=names, weights=weights)
            got = check_records(call(hip, s, kind, n, names=names, weights=weights), ld_v, n, f"E={E} {kind} n={n} {names} {weights}")
            if E > 1 and n > 1 and weights == "negative":
                assert got[0, 0] < 0.0 < got[1, 0]                            # a negative borrowing spread: a negative cost
    print(f"E={E} {kind}: largest yardstick {worst[0]:.3e}, largest per-path gap {worst[1]:.3e}")


@pytest.mark.parametrize("kind", KINDS)
def test_unit_weights_without_names_are_the_sequential_sums(kind, hip, setups):
    """every product is exact (S = 1, phi = 1), so per path fca is the float64 sum of relu(x_k) in date order, bit for bit"""
    s = setups[11]
    dev = one_path_calls(hip, s, kind, "none", "unit")
    x = mr.unsecured_np(s["expo"], *s["desc"][kind])
    fca, fba = np.zeros(N_MAX), np.zeros(N_MAX)
    for k in range(x.shape[0] - 1):
        fca = fca + np.maximum(x[k], 0.0)
        fba = fba + np.maximum(-x[k], 0.0)
    assert fca.any() and fba.any()
    assert dev[0].tobytes() == fca.tobytes() and dev[1].tobytes() == fba.tobytes() and dev[2].tobytes() == (fca - fba).tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_identities(kind, hip, setups):
    s, n = setups[11], N_MAX
    rec = call(hip, s, kind, n)
    full = stats(rec)
    assert full[0, 0] > 0.0 and full[1, 0] > 0.0
    # two calls, identical bytes
    assert call(hip, s, kind, n).tobytes() == rec.tobytes()
    # the two names swapped: w = S_c * S_o commutes, no byte changes
    assert call(hip, s, kind, n, swap_names=True).tobytes() == rec.tobytes()
    for names in ("cp", "own"):
        assert call(hip, s, kind, n, names=names, swap_names=True).tobytes() == call(hip, s, kind, n, names=names).tobytes()
    # weight tables swapped, exposures negated: the same arithmetic on the other accumulator
    r = call(hip, s, kind, n, negate=True, swap_weights=True)
    assert r[0].tobytes() == rec[1].tobytes() and r[1].tobytes() == rec[0].tobytes()
    assert r[2]["n"] == rec[2]["n"] and r[2]["shift"] == -rec[2]["shift"] and r[2]["s1"] == -rec[2]["s1"] and r[2]["s2"] == rec[2]["s2"]
    # all-zero lending weights: fba == 0 exactly, fva == fca bit for bit
    r = call(hip, s, kind, n, weights="zero lend")
    assert r[1].tobytes() == np.array([(float(n), 0.0, 0.0, 0.0)], dtype=_abi.ACC_DTYPE).tobytes()
    assert r[2].tobytes() == r[0].tobytes() == rec[0].tobytes()
    # a survival probability only shrinks a leg
    none = stats(call(hip, s, kind, n, names="none"))
    assert 0.0 < full[0, 0] < none[0, 0] and 0.0 < full[1, 0] < none[1, 0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("E", [2, 11])
def test_unit_weights_without_names_sum_the_profiles(E, kind, hip, setups):
    """fca / fba means == sum over k < E-1 of the EPE / ENE means of mcx_reduce_profiles on the same exposures"""
    s, n = setups[E], N_MAX
    got = stats(call(hip, s, kind, n, names="none", weights="unit"))
    prof = hip.reduce_profiles(UnsecuredSpec(*s["desc"][kind]), place(hip, s["expo"], n)).view(np.float64).reshape(E, 2, 4)
    epe = sum(mean_and_error(prof[k, 0])[0] for k in range(E - 1))
    ene = sum(mean_and_error(prof[k, 1])[0] for k in range(E - 1))              # (the ENE records hold -relu(-x))
    print(f"E={E} {kind}: fca {got[0, 0]:.17e} sum EPE {epe:.17e}; fba {got[1, 0]:.17e} -sum ENE {-ene:.17e}")
    assert epe > 0.0 > ene
    assert np.isclose(got[0, 0], epe, rtol=1e-12, atol=0.0) and np.isclose(got[1, 0], -ene, rtol=1e-12, atol=0.0)


def test_grid_stride(hip, setups):
    """(block cap x 256 + 257) paths at E = 2: every block takes a second path in the stride, one more block's worth and a partial one.
    The 513-path inputs tiled; against the restatement of the tiled integrands and against its own two halves merged"""
    s, kind = setups[2], "mpor"
    cap = 8 * hip.device_info()["n_cu"]
    n = cap * 256 + 257
    reps = -(-n // N_MAX)
    expo = hip.from_numpy(np.tile(s["expo"], (1, reps))[:, :n].copy())
    paths = hip.from_numpy(np.tile(s["paths"], (1, 1, reps))[:, :, :n].copy())
    wb, wl = s["weights"]["curves"]
    u = UnsecuredSpec(*s["desc"][kind])
    rec = hip.reduce_fva(s["book"], u, s["cp"], s["own"], wb, wl, expo, paths)
    assert rec.tobytes() == hip.reduce_fva(s["book"], u, s["cp"], s["own"], wb, wl, expo, paths).tobytes()
    _, ld513 = reference(s, kind, N_MAX)
    ld = np.tile(ld513, (1, reps))[:, :n]
    print(f"grid stride: {n} paths, cap {cap} blocks")
    full = check_records(rec, ld, n, f"grid stride n={n}")
    half = n // 2 + 3                                                            # (an odd cut: the second half is a path-sliced view)
    parts = [hip.reduce_fva(s["book"], u, s["cp"], s["own"], wb, wl, expo[:, a:b], paths[:, :, a:b]) for a, b in ((0, half), (half, n))]
    for e in range(3):
        N, mean, M2 = combine_acc(np.array([[p[e]["n"], p[e]["shift"], p[e]["s1"], p[e]["s2"]] for p in parts]))
        err = np.sqrt(M2 / (N - 1.0)) / np.sqrt(N)
        assert N == float(n) and np.isclose(mean, full[e, 0], rtol=1e-12, atol=0.0) and np.isclose(err, full[e, 1], rtol=1e-9, atol=0.0)


def raw_args(hip, s, kind="mpor", n=N_MAX):
    u = UnsecuredSpec(*s["desc"][kind])
    expo, paths = place(hip, s["expo"], n), place(hip, s["paths"], n)
    u.desc.n_rows = expo.shape[0]
    ids = [np.ascontiguousarray(x, dtype=np.int32) for x in (s["cp"], s["own"])]
    w = [np.ascontiguousarray(x, dtype=np.float64) for x in s["weights"]["curves"]]
    keep = (u, expo, paths, ids, w)
    args = dict(h=hip.h, book=s["book"].ptr, u=C.byref(u.desc), sc=_abi.ptr(ids[0]), so=_abi.ptr(ids[1]), wb=_abi.ptr(w[0]), wl=_abi.ptr(w[1]),
                expo=C.c_void_p(expo.data_ptr()), paths=C.c_void_p(paths.data_ptr()), n=C.c_int64(n), ld_expo=C.c_int64(n + PAD),
                ld_paths=C.c_int64(n + PAD))
    return args, keep


ORDER = ("h", "book", "u", "sc", "so", "wb", "wl", "expo", "paths", "n", "ld_expo", "ld_paths")


def raw_call(hip, args, out):
    return hip.lib.mcx_reduce_fva(*[args[k] for k in ORDER], _abi.ptr(out), hip._stream())


def test_refusals_leave_the_output_untouched(hip, setups):
    s = setups[11]
    args, keep = raw_args(hip, s)
    poison = np.frombuffer(b"\xab" * (3 * 32), dtype=_abi.ACC_DTYPE).copy()
    null = C.c_void_p(0)

    def bad_ids(which, value):
        ids = np.array(keep[3][which], copy=True)
        ids[len(ids) // 2] = value
        return ids

    def bad_desc(rows=None, delayed=None, n_rows=None, n_dates=None):
        r0, d0, h, coll = s["desc"]["mpor"]
        u = UnsecuredSpec(r0 if rows is None else rows, d0 if delayed is None else delayed, h, coll)
        u.desc.n_rows = keep[1].shape[0] if n_rows is None else n_rows
        if n_dates is not None:
            u.desc.n_dates = n_dates
        return u

    rows_hi, del_hi = s["desc"]["mpor"][0].copy(), s["desc"]["mpor"][1].copy()
    rows_hi[3], del_hi[5] = keep[1].shape[0], keep[1].shape[0]
    rows_neg = s["desc"]["mpor"][0].copy()
    rows_neg[2] = -1
    cases_ = [("handle", dict(h=null), -1), ("book", dict(book=null), -1), ("descriptor", dict(u=null), -1), ("expo", dict(expo=null), -1),
              ("paths", dict(paths=null), -1), ("borrowing weights", dict(wb=null), -1), ("lending weights", dict(wl=null), -1),
              ("ld_expo", dict(ld_expo=C.c_int64(N_MAX - 1)), -2), ("ld_paths", dict(ld_paths=C.c_int64(N_MAX - 1)), -2)]
    for which, key in enumerate(("sc", "so")):
        for value in (-1, 1 << 20):
            cases_.append((f"atom id {value} in {key}", {key: bad_ids(which, value)}, -2))
    for tag, u in (("row beyond the block handed over", bad_desc(rows=rows_hi)), ("negative row", bad_desc(rows=rows_neg)),
                   ("delayed row beyond the block", bad_desc(delayed=del_hi)),
                   ("row beyond the book's exposure rows", bad_desc(rows=rows_hi, n_rows=keep[1].shape[0] + 1)),
                   ("delayed row beyond the book's exposure rows", bad_desc(delayed=del_hi, n_rows=keep[1].shape[0] + 1)),
                   ("no dates", bad_desc(n_dates=0)), ("too many dates", bad_desc(n_dates=513))):
        cases_.append((tag, dict(u=u), -2))
    for tag, override, code in cases_:
        a = dict(args)
        for k, v in override.items():
            a[k] = _abi.ptr(v) if isinstance(v, np.ndarray) else C.byref(v.desc) if isinstance(v, UnsecuredSpec) else v
        out = poison.copy()
        rc = raw_call(hip, a, out)
        assert rc == code and out.tobytes() == poison.tobytes(), (tag, rc)
        if tag != "handle":                                                      # each refusal says why
            msg = (hip.lib.mcx_last_error(hip.h) or b"").decode()
            assert "mcx_reduce_fva" in msg or "unsecured desc" in msg, (tag, msg)
    assert hip.lib.mcx_reduce_fva(*[args[k] for k in ORDER], null, hip._stream()) == -1
    # the workspace: more partials than it holds cannot be asked for through the ABI (the grid is capped at 8 blocks per CU, 96 KiB
    # of partials against 8 MiB), so that refusal has no case here
    # and the unchanged arguments are accepted
    out = poison.copy()
    assert raw_call(hip, args, out) == 0 and out.tobytes() == call(hip, s, "mpor", N_MAX).tobytes()


def test_no_paths_zeroes_the_output(hip, setups):
    args, keep = raw_args(hip, setups[11])
    for n in (0, -3):
        out = np.frombuffer(b"\xab" * (3 * 32), dtype=_abi.ACC_DTYPE).copy()
        assert raw_call(hip, dict(args, n=C.c_int64(n)), out) == 0 and out.tobytes() == bytes(3 * 32)
