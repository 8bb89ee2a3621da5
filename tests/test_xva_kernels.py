"""k4_xva (csrc/k4_xva.hip) through the C ABI, mcx_reduce_xva: per-path integrands and reduced records against the numpy restatement
of the table (tests/xva_reference.py), the identities between the five evaluations, every refusal.

Inputs come from small compiled controllers (payer swap under ModelConfig[Vasicek, CIR++(cp), CIR++(own)], all three correlated,
tests/xva_cases.py): the exposure block, the paths, the book and its atoms.  They are re-placed in tensors with a padded leading
dimension and NaN beyond the n paths of a case, so an over-read poisons a sum.  The restatement is fed the unsecured exposures
(tests/metric_reference.unsecured_np, bit-equal to the oracle's) and the four atom value arrays as mcx_resolve_atoms gives them on
the device — the same dev_atom the kernel inlines, tied here to the oracle's atoms at 1e-13 — so what is compared is the table's
arithmetic and the reduction, not two exponentials.

Bounds.  Per path: the yardstick of a case is the restatement's own float64-against-long-double gap over the case's largest
integrand; the device must sit within max(4 x yardstick, E x 2.2e-16) of the long-double restatement.  Records: mean at rtol 1e-12,
error at rtol 1e-9 (the bounds of tests/test_plugin_metrics.py for CVA).  The test prints each case's figures before it asserts;
the figures measured on the MI355X are in README "Bilateral xVA".

One launch shape (grid-stride above 8 blocks per CU), so there is no second kernel to test."""
import ctypes as C

import numpy as np
import pytest
import torch

import metric_reference as mr
import xva_cases as xc
import xva_reference as xr
from mcx import _abi
from mcx.metrics.bcva_metric import BilateralCVAMetric
from mcx.metrics.metric import mean_and_error
from mcx.plan import UnsecuredSpec

pytestmark = pytest.mark.gpu

TIMELINES = {1: np.array([0.5]), 2: np.array([0.5, 1.0]), 11: xc.TIMELINE}
N_MAX, COUNTS, PAD = 513, (1, 255, 257, 513), 7
KINDS = ("plain", "threshold", "mpor")


def place(be, mat, n):
    """mat [..][>= n] -> device view [..][n] of a NaN-filled buffer with leading dimension n + PAD"""
    lead, ld = mat.shape[:-1], n + PAD
    buf = np.full(lead + (ld,), np.nan)
    buf[..., :n] = mat[..., :n]
    return be.from_numpy(buf)[..., :n]


@pytest.fixture(scope="module")
def setups(hip, oracle):
    """E -> the compiled controller's book, atoms, exposure block and paths (numpy), the three descriptors"""
    out = {}
    for E, tl in TIMELINES.items():
        sc = xc.controller(hip, [BilateralCVAMetric("cp", "own", xc.R_CP, xc.R_OWN)], n_main=N_MAX, n_pre=1024, timeline=tl,
                           threshold=xc.THRESHOLD, mpor=xc.MPOR)
        sc.run_simulation()
        (cp, _), (own, _) = sc._xva_atoms[0]
        paths, expo = sc.last_state["paths"], sc.last_state["expo"][0]
        ids = list(cp[0]) + list(cp[1]) + list(own[0]) + list(own[1])
        if ids:
            at = hip.resolve_atoms(sc.book, ids, paths.contiguous()).cpu().numpy().reshape(4, E - 1, N_MAX)
            at_o = oracle.resolve_atoms(sc.book, ids, paths.cpu().contiguous()).numpy().reshape(4, E - 1, N_MAX)
            assert np.allclose(at, at_o, rtol=1e-13, atol=0.0)
        else:
            at = np.zeros((4, 0, N_MAX))
        rows, delayed = sc.metric_exposure_indices.numpy(), sc.netting_set_delayed_exposure_indices[0].numpy()
        out[E] = dict(sc=sc, book=sc.book, cp=cp, own=own, atoms=at, paths=paths.cpu().numpy(), expo=expo.cpu().numpy(),
                      desc={"plain": (rows, None, 0.0, False), "threshold": (rows, None, xc.THRESHOLD, False),
                            "mpor": (rows, delayed, xc.THRESHOLD, True)})
    return out


def reference(s, kind, n, cp=True, own=True, negate=False, dtype=np.longdouble):
    x = mr.unsecured_np(-s["expo"] if negate else s["expo"], *s["desc"][kind])[:, :n]
    a = s["atoms"][:, :, :n]
    return x, xr.integrands(x, a[0] if cp else None, a[1] if cp else None, a[2] if own else None, a[3] if own else None,
                            xc.R_CP, xc.R_OWN, dtype=dtype)


def call(hip, s, kind, n, cp=True, own=True, negate=False, swap=False):
    """records [5] of the first n paths"""
    expo = place(hip, -s["expo"] if negate else s["expo"], n)
    paths = place(hip, s["paths"], n)
    a, b = (s["cp"] if cp else None, xc.R_CP), (s["own"] if own else None, xc.R_OWN)
    if swap:
        a, b = b, a
    return hip.reduce_xva(s["book"], UnsecuredSpec(*s["desc"][kind]), a[0], a[1], b[0], b[1], expo, paths)


def stats(rec):
    return np.array([mean_and_error(np.array([r["n"], r["shift"], r["s1"], r["s2"]])) for r in rec])


@pytest.fixture(scope="module")
def per_path(hip, setups):
    """(E, kind) -> [5][N_MAX] device integrands: the shift of the record of a one-path call"""
    out = {}
    for E, s in setups.items():
        expo, paths = place(hip, s["expo"], N_MAX), place(hip, s["paths"], N_MAX)
        for kind in KINDS:
            v = np.zeros((5, N_MAX))
            u = UnsecuredSpec(*s["desc"][kind])
            for i in range(N_MAX):
                rec = hip.reduce_xva(s["book"], u, s["cp"], xc.R_CP, s["own"], xc.R_OWN, expo[:, i:i + 1], paths[:, :, i:i + 1])
                assert np.all(rec["n"] == 1.0) and np.all(rec["s1"] == 0.0) and np.all(rec["s2"] == 0.0)
                v[:, i] = rec["shift"]
            out[E, kind] = v
    return out


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
        assert np.all(rec["n"] == float(n)) and np.array_equal(rec["shift"], dev[:, 0])
        got = stats(rec)
        m_ref, e_ref = (np.asarray(t, dtype=np.float64) for t in xr.mean_and_error(ld))
        print(f"E={E} {kind} n={n}: mean off {np.abs(got[:, 0] - m_ref).max():.3e}, error off "
              f"{0.0 if n == 1 else np.abs(got[:, 1] - e_ref).max():.3e}")
        assert np.allclose(got[:, 0], m_ref, rtol=1e-12, atol=0.0), (E, kind, n, got[:, 0], m_ref)
        assert np.allclose(got[:, 1], e_ref, rtol=1e-9, atol=0.0, equal_nan=True), (E, kind, n, got[:, 1], e_ref)
        if E == 1 and n > 1:
            assert not got.any()                                              # exactly (0, 0), five times
    print(f"E={E} {kind}: largest yardstick {worst[0]:.3e}, largest per-path gap {worst[1]:.3e}")


@pytest.mark.parametrize("kind", KINDS)
def test_identities(kind, hip, setups):
    s, n = setups[11], N_MAX
    rec = call(hip, s, kind, n)
    full = stats(rec)
    # (e) two calls, identical bytes
    assert call(hip, s, kind, n).tobytes() == rec.tobytes()
    # (a) no own name: cva and cva_ftd are mcx_reduce_cva's record
    r = stats(call(hip, s, kind, n, own=False))
    cva = stats(hip.reduce_cva(s["book"], UnsecuredSpec(*s["desc"][kind]), s["cp"][0], s["cp"][1], xc.R_CP, place(hip, s["expo"], n),
                               place(hip, s["paths"], n)))[0]
    for e in (0, 2):
        assert np.isclose(r[e, 0], cva[0], rtol=1e-12, atol=0.0) and np.isclose(r[e, 1], cva[1], rtol=1e-9, atol=0.0)
    assert np.isclose(full[0, 0], cva[0], rtol=1e-12, atol=0.0) and r[1, 0] == 0.0 and r[3, 0] == 0.0
    # (b) no counterparty: cva == 0 exactly, dva_ftd == dva bit for bit
    r = call(hip, s, kind, n, cp=False)
    assert r[0].tobytes() == np.array([(float(n), 0.0, 0.0, 0.0)], dtype=_abi.ACC_DTYPE).tobytes() == r[2].tobytes()
    assert r[3].tobytes() == r[1].tobytes() and stats(r)[1, 0] > 0.0
    # (c) exposures negated, names swapped: the same arithmetic on the other accumulator
    r = call(hip, s, kind, n, negate=True, swap=True)
    for a, b in ((0, 1), (1, 0), (2, 3), (3, 2)):
        assert r[a].tobytes() == rec[b].tobytes(), (a, b)
    assert r[4]["n"] == rec[4]["n"] and r[4]["shift"] == -rec[4]["shift"] and r[4]["s1"] == -rec[4]["s1"] and r[4]["s2"] == rec[4]["s2"]
    # (d) a survival probability only shrinks a leg
    assert 0.0 < full[2, 0] < full[0, 0] and 0.0 < full[3, 0] < full[1, 0]


def raw_args(hip, s, kind="mpor", n=N_MAX):
    u = UnsecuredSpec(*s["desc"][kind])
    expo, paths = place(hip, s["expo"], n), place(hip, s["paths"], n)
    u.desc.n_rows = expo.shape[0]
    ids = [np.ascontiguousarray(x, dtype=np.int32) for x in (s["cp"][0], s["cp"][1], s["own"][0], s["own"][1])]
    keep = (u, expo, paths, ids)
    args = dict(h=hip.h, book=s["book"].ptr, u=C.byref(u.desc), sc=_abi.ptr(ids[0]), cc=_abi.ptr(ids[1]), rc=C.c_double(xc.R_CP),
                so=_abi.ptr(ids[2]), co=_abi.ptr(ids[3]), ro=C.c_double(xc.R_OWN), expo=C.c_void_p(expo.data_ptr()),
                paths=C.c_void_p(paths.data_ptr()), n=C.c_int64(n), ld_expo=C.c_int64(n + PAD), ld_paths=C.c_int64(n + PAD))
    return args, keep


def raw_call(hip, args, out):
    return hip.lib.mcx_reduce_xva(*[args[k] for k in ("h", "book", "u", "sc", "cc", "rc", "so", "co", "ro", "expo", "paths", "n",
                                                       "ld_expo", "ld_paths")], _abi.ptr(out), hip._stream())


def test_refusals_leave_the_output_untouched(hip, setups):
    s = setups[11]
    args, keep = raw_args(hip, s)
    poison = np.frombuffer(b"\xab" * (5 * 32), dtype=_abi.ACC_DTYPE).copy()
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
              ("paths", dict(paths=null), -1), ("ld_expo", dict(ld_expo=C.c_int64(N_MAX - 1)), -2),
              ("ld_paths", dict(ld_paths=C.c_int64(N_MAX - 1)), -2), ("half a pair, cp", dict(cc=null), -2),
              ("half a pair, own", dict(so=null), -2)]
    for which, key in enumerate(("sc", "cc", "so", "co")):
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
    a = dict(args)
    assert hip.lib.mcx_reduce_xva(*[a[k] for k in ("h", "book", "u", "sc", "cc", "rc", "so", "co", "ro", "expo", "paths", "n", "ld_expo",
                                                    "ld_paths")], null, hip._stream()) == -1
    # and the unchanged arguments are accepted
    out = poison.copy()
    assert raw_call(hip, args, out) == 0 and out.tobytes() == call(hip, s, "mpor", N_MAX).tobytes()


def test_no_paths_zeroes_the_output(hip, setups):
    args, keep = raw_args(hip, setups[11])
    for n in (0, -3):
        out = np.frombuffer(b"\xab" * (5 * 32), dtype=_abi.ACC_DTYPE).copy()
        assert raw_call(hip, dict(args, n=C.c_int64(n)), out) == 0 and out.tobytes() == bytes(5 * 32)
