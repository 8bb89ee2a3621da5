"""The metric kernels at kernel level: csrc/k4_reduce.hip (k4_vector, k4_profiles, k4_cva_paths, k4_cva_paths_v<2>, k4_unsecured),
k_finish_acc (csrc/mcx_api.hip) and csrc/k5_select.hip (k5_hist<false>, k5_hist<true>, k5_bracket<true>, k5_bracket<false>,
k5_narrow), called through the backend methods and compared with the plain numpy references of tests/metric_reference.py.

The references are pinned to the CPU oracle first (tests without the gpu mark).  The GPU tests then check RAW kernel outputs —
records, histograms, `below` / `count` / candidate rows — because the drivers above them hide a wrong one: _select_with_bracket
redoes by digit passes any date whose bracket counts look wrong, and a mean at 10^6 paths moves by 1e-6 relative for one dropped
element.  Every exposure matrix here has NaN in its pad columns and in the rows no descriptor names: an over-read poisons a sum
or shows up as a NaN key.

NaNs that ARITHMETIC produces (inf - inf, x - NaN) have a sign IEEE 754 leaves open, and the sign decides the key of the NaN.  The
collateralised special-value data therefore keeps NaN and inf out of the rows used as `delayed`: e - coll then either is finite,
an inf, or returns e's own NaN."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import cases
import metric_reference as mr

from mcx import _abi
from mcx.controller.controller import _SELECT_DIGITS
from mcx.metrics.metric import combine_acc, mean_and_error
from mcx.plan import UnsecuredSpec

gpu = pytest.mark.gpu
U = 2.0 ** -53
LOST = int(_abi.SELECT_LOST)
DIGITS = tuple(_SELECT_DIGITS) + ((0, 1), (63, 1))

# ---- data -------------------------------------------------------------------------------------------------------------------------
# exposure matrices of 7 rows: E_ROWS may hold any special value, D_ROWS (the rows `delayed` points at) only finite ones, row 4 is
# named by no descriptor and is NaN throughout
E_ROWS, D_ROWS, UNNAMED, N_ROWS = (0, 2, 3, 5), (1, 6), 4, 7
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 1.1e-308, -1.1e-308, 1e300, -1e300, 0.25, -0.25, 0.1, 1.0])
FINITE_SPECIALS = np.array([0.0, -0.0, 5e-324, -5e-324, 1.1e-308, -1.1e-308, 0.25, -0.25, 0.1, 1e300])


def special_matrix(n, seed):
    """[7][n]: normal, heavily tied, tiny / denormal and heavy-tailed rows with NaN, +-inf, +-0 and denormals sprinkled in"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N_ROWS, n))
    x[2] = np.round(x[2], 1)
    x[3, : n // 2] *= 1e-307
    x[5] = np.exp(3.0 * x[5]) * np.sign(x[0])
    x[6] *= 0.5
    for r in range(N_ROWS):
        k = max(1, n // 5)
        idx = rng.permutation(n)[:k]
        pool = FINITE_SPECIALS if r in D_ROWS else SPECIALS
        x[r, idx] = pool[(np.arange(k) + r) % len(pool)]
    x[UNNAMED] = np.nan
    return x


def integer_matrix(n, seed):
    """[7][n] integer-valued doubles, |x| <= 1000; row 4 NaN"""
    x = np.random.default_rng(seed).integers(-1000, 1001, size=(N_ROWS, n)).astype(np.float64)
    x[UNNAMED] = np.nan
    return x


def descriptors(E, h):
    """three descriptors of E dates: rows permuted and repeated; `delayed` mixing -1 and valid rows"""
    named = E_ROWS + D_ROWS
    rows = np.array([named[(5 * m + m // 6 + 1) % 6] for m in range(E)])
    rows_c = np.array([E_ROWS[(3 * m + m // 4 + 1) % 4] for m in range(E)])
    delayed = np.array([(-1, D_ROWS[0], D_ROWS[1])[(m + m // 3) % 3] for m in range(E)])
    return {"plain": (rows, None, 0.0, False), "threshold": (rows, None, h, False), "collateralised": (rows_c, delayed, h, True)}


def place(be, mat, ld, offset=0, wider=0):
    """mat [R][n] -> backend view [R][n + wider] of a NaN-filled flat buffer: leading dimension ld, base `offset` doubles in"""
    R, n = mat.shape
    assert ld >= n + wider
    buf = np.full(R * ld + offset, np.nan)
    buf[offset:].reshape(R, ld)[:, :n] = mat
    t = be.from_numpy(buf)
    return t[offset:offset + R * ld].view(R, ld)[:, :n + wider]


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def values_equal(a, b):
    """equal as np.sort orders them: -0.0 == +0.0 (np.sort leaves their order open, the key puts -0.0 first), NaN == NaN (np.sort
    puts NaN last, where the key of a positive NaN sits)"""
    return np.array_equal(a, b, equal_nan=True)


def int_record(v):
    """exact integer record of an integer-valued vector"""
    d = (v - v[0]).astype(np.int64)
    return float(len(v)), float(v[0]), float(d.sum()), float((d * d).sum())


def assert_record(rec, n, shift, s1, s2, tag):
    got = (float(rec["n"]), float(rec["shift"]), float(rec["s1"]), float(rec["s2"]))
    assert got == (n, shift, s1, s2), (tag, got, (n, shift, s1, s2))


def profile_records_int(u):
    """expected [E][2] records (positive part, negative part) of integer-valued unsecured exposures"""
    p, q = mr.relu_parts(u)
    return [[int_record(p[m]), int_record(q[m])] for m in range(u.shape[0])]


# =====================================================================================================================================
# CPU: the references against the oracle (and against exact rational arithmetic)
# =====================================================================================================================================
N_CPU = 4099


@pytest.mark.parametrize("kind", ["plain", "threshold", "collateralised"])
def test_reference_unsecured_equals_oracle(kind, oracle):
    """unsecured_np == orc_unsecured bit for bit on the special-value matrix (NaN, +-inf, +-0, denormals), n = 4099"""
    x = special_matrix(N_CPU, 1)
    rows, delayed, h, coll = descriptors(9, 0.25)[kind]
    got = oracle.unsecured(UnsecuredSpec(rows, delayed, h, coll), torch.from_numpy(x)).numpy()
    assert bits_equal(got, mr.unsecured_np(x, rows, delayed, h, coll))


@pytest.mark.parametrize("n_sel", [1, 3, 4])
@pytest.mark.parametrize("kind", ["plain", "threshold", "collateralised"])
def test_reference_hist_equals_oracle_on_all_six_passes(kind, n_sel, oracle):
    """hist_np == orc_select_hist on each of the six digit passes of a select (the prefixes narrowed by narrow_np as it goes), and
    the walk ends at the order statistics of np.sort: pins key_np, hist_np, narrow_np and key_to_double_np together"""
    x = special_matrix(N_CPU, 2)
    rows, delayed, h, coll = descriptors(5, 0.25)[kind]
    unsec = UnsecuredSpec(rows, delayed, h, coll)
    u = mr.unsecured_np(x, rows, delayed, h, coll)
    ranks = [0, N_CPU // 3, N_CPU // 3 + 1, N_CPU - 1][:n_sel]
    prefix = np.zeros((5, n_sel), dtype=np.uint64)
    rem = np.tile(np.asarray(ranks, dtype=np.int64), (5, 1))
    for shift, bits in _SELECT_DIGITS:
        ref = mr.hist_np(u, prefix, shift, bits)
        got = oracle.select_hist(unsec, torch.from_numpy(x), n_sel, prefix, shift, bits).numpy()
        assert np.array_equal(got, ref), (shift, bits)
        prefix, rem = mr.narrow_np(ref, prefix, rem, shift)
    assert values_equal(mr.key_to_double_np(prefix), np.sort(u, axis=1)[:, ranks])


def test_reference_order_statistics_equal_oracle_sort(oracle):
    """np.sort of unsecured_np == orc_pfe_sort at q - 1, q, q + 1 (threshold descriptor: it maps the NaNs to 0, so the oracle's
    comparison sort is well defined; +-inf, +-0 and denormals stay)"""
    x = special_matrix(N_CPU, 3)
    rows, delayed, h, coll = descriptors(5, 0.25)["threshold"]
    u = mr.unsecured_np(x, rows, delayed, h, coll)
    for q in (1, N_CPU // 2, N_CPU - 2):
        got = oracle.pfe_sort(UnsecuredSpec(rows, delayed, h, coll), torch.from_numpy(x), q)
        assert np.array_equal(got, np.sort(u, axis=1)[:, [q - 1, q, q + 1]]), q


@pytest.mark.parametrize("kind", ["plain", "threshold", "collateralised"])
def test_reference_profiles_equal_oracle_exactly(kind, oracle):
    """integer-valued exposures (every partial sum exact) with NaN and +-0 sprinkled in: the oracle's records equal the integer
    sums of relu_parts(unsecured_np) exactly, n = 4099"""
    x = integer_matrix(N_CPU, 4)
    rng = np.random.default_rng(5)
    for r in E_ROWS:
        x[r, rng.permutation(N_CPU)[:300]] = np.array([np.nan, 0.0, -0.0])[np.arange(300) % 3]
    rows, delayed, h, coll = descriptors(9, 3.0)[kind]
    u = mr.unsecured_np(x, rows, delayed, h, coll)
    if kind != "threshold":
        assert np.isnan(u).any()
    got = oracle.reduce_profiles(UnsecuredSpec(rows, delayed, h, coll), torch.from_numpy(x))
    exp = profile_records_int(np.where(np.isnan(u), 0.0, u))
    for m in range(9):
        for s in range(2):
            assert_record(got[m, s], *exp[m][s], (m, s))
    v = x[0, :N_CPU].copy()
    v[np.isnan(v)] = 7.0
    assert_record(oracle.reduce_vector(torch.from_numpy(v))[0], *int_record(v), "vector")


def test_acc_exact_against_rational_arithmetic():
    """the Veltkamp-split fsum of acc_exact is the exact sum: equal to fractions.Fraction on full-mantissa data"""
    rng = np.random.default_rng(6)
    v = 1e6 + rng.standard_normal(257) * np.exp(rng.standard_normal(257) * 5.0)
    a = mr.acc_exact(v)
    d = [Fraction(float(t - v[0])) for t in v]
    assert a["s1"] == float(sum(d)) and a["s2"] == float(sum(t * t for t in d)) and a["abs1"] == float(sum(abs(t) for t in d))
    assert (a["n"], a["shift"]) == (257.0, v[0])


def test_combine_acc_against_long_double():
    """records of different shifts and sizes, one with n = 0: (N, mean, M2) of the concatenation in long double"""
    rng = np.random.default_rng(7)
    parts = [1e6 + rng.standard_normal(1000), np.zeros(0), 1e6 + 3.0 + 2.0 * rng.standard_normal(37), np.array([1e6 - 50.0]),
             1e6 + rng.standard_normal(4099) * 0.01]
    recs = np.zeros(len(parts), dtype=_abi.ACC_DTYPE)
    for k, p in enumerate(parts):
        a = mr.acc_exact(p)
        recs[k] = (a["n"], a["shift"] if len(p) else 123.0, a["s1"], a["s2"])
    N, mean, M2 = combine_acc(recs.view(np.float64))
    allv = np.concatenate(parts)
    m_ref, e_ref, m2_ref = mr.mean_err_longdouble(allv)
    assert N == len(allv)
    assert abs(mean - m_ref) <= 1e-15 * abs(m_ref)
    assert abs(M2 - m2_ref) <= 1e-9 * m2_ref              # (s2 - s1^2/n per record: ~1e-12 here, shifts sit inside the data)
    val, err = mean_and_error(recs.view(np.float64))
    assert val == mean and abs(err - e_ref) <= 1e-9 * e_ref
    assert combine_acc(recs[1:2].view(np.float64)) == (0.0, 0.0, 0.0)


# =====================================================================================================================================
# K4 on the GPU
# =====================================================================================================================================
N_INT = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 262143, 262144, 262145, (1 << 20) + 3]


def _lds(n):
    from mcx._native import padded_ld
    return sorted({n + 5, padded_ld(n)} - {n})


@gpu
@pytest.mark.parametrize("n", N_INT)
def test_reduce_vector_integer_exact(n, hip):
    """k4_vector + k_finish_acc: one block per 256 paths up to 262144 = MCX_MAX_PARTIAL_BLOCKS * 256 paths, a strided loop beyond
    (262145, 2^20 + 3); n < 64 leaves lanes of the only wave idle.  Integer data: shift, s1, s2, n equal the integer sums whatever
    the order.  The vector is an unaligned slice of a NaN buffer."""
    x = integer_matrix(n, 10 + n % 97)[0]
    buf = np.full(n + 8, np.nan)
    buf[3:3 + n] = x
    rec = hip.reduce_vector(hip.from_numpy(buf)[3:3 + n])[0]
    assert_record(rec, *int_record(x), n)


@gpu
@pytest.mark.parametrize("n", N_INT)
def test_reduce_profiles_integer_exact(n, hip):
    """k4_profiles + k_finish_acc, grid (chunks, E) with chunks = min(ceil(n / 1024), 8 n_cu / min(E, 8) + 1): E = 9 dates, rows
    permuted and repeated, at every n of the vector test (one chunk up to 1024 paths; at 2^20 + 3 the chunk loop strides for
    E >= 8), plus E in {1, 8, 9, 512} where the grid formula changes (n = 1000: one chunk; n = 4099: five; 2^20 + 3: E = 1 does
    not stride, E = 8 and 9 do).  Plain, threshold and collateralised (delayed mixing -1 and valid rows), ld = n + 5 and padded_ld;
    pads and the unnamed row are NaN."""
    x = integer_matrix(n, 20 + n % 89)
    Es = {9}
    if n in (1000, (1 << 20) + 3):
        Es |= {1, 8}
    sweeps = [(x, Es)]
    if n == 1000:
        sweeps = [(x, Es | {512}), (integer_matrix(4099, 21), {1, 8, 9, 512})]
    for mat, es in sweeps:
        nn = mat.shape[1]
        for ld in _lds(nn):
            expo = place(hip, mat, ld)
            for E in sorted(es):
                for kind, (rows, delayed, h, coll) in descriptors(E, 3.0).items():
                    got = hip.reduce_profiles(UnsecuredSpec(rows, delayed, h, coll), expo)
                    exp = profile_records_int(mr.unsecured_np(mat, rows, delayed, h, coll))
                    for m in range(E):
                        for s in range(2):
                            assert_record(got[m, s], *exp[m][s], (nn, ld, E, kind, m, s))


@gpu
def test_too_many_metric_dates_are_rejected_on_the_host(hip):
    """E = 513 > MCX_MAX_METRIC_DATES fails in mcx_upload_unsec, before any launch"""
    from mcx._native import McxError
    x = place(hip, integer_matrix(64, 30), 69)
    with pytest.raises(McxError, match="n_dates 513 out of range"):
        hip.reduce_profiles(UnsecuredSpec(np.zeros(513, dtype=np.int32), None, 0.0, False), x)
    with pytest.raises(McxError, match="n_dates 513 out of range"):
        hip.select_hist(UnsecuredSpec(np.zeros(513, dtype=np.int32), None, 0.0, False), x, 1, np.zeros((513, 1), dtype=np.uint64), 53, 11)


def _float_sets(n):
    rng = np.random.default_rng(40)
    base = 1e6 + rng.standard_normal(n)
    outlier = base.copy()
    outlier[0] = 1e6 + 1e4                                # the shift of the record: 1e4 sigma off the mean
    return {"smooth": base, "outlier": outlier, "constant": np.full(n, 1e6 + 0.125)}


@gpu
@pytest.mark.parametrize("n", [4099, 300001])
def test_reduce_floating_data_within_summation_bounds(n, hip):
    """k4_vector (4099: 17 blocks; 300001: the strided loop of 1024 blocks) and k4_profiles on 1e6 + N(0,1), the same with a first
    path 1e4 sigma out (the record's shift) and a constant row.  Bounds valid for ANY summation order over d = fl(x - x[0]):
    |s1 - exact| <= n u sum|d|, |s2 - exact| <= (n + 3) u sum d^2.  The constant row gives s1 == s2 == 0.0 and an error of 0.0.
    mean_and_error against the long-double two-pass figures at the project's rtol (1e-8 value, 1e-6 error); for the outlier the
    error tolerance is what the two bounds allow for M2 = s2 - s1^2 / n (derived below)."""
    sets = _float_sets(n)
    mat = np.stack(list(sets.values()) + [np.full(n, np.nan)])
    expo = place(hip, mat, n + 5)
    prof = hip.reduce_profiles(UnsecuredSpec(np.array([2, 0, 1, 0]), None, 0.0, False), expo)
    order = {"constant": 0, "smooth": 1, "outlier": 2}
    for name, v in sets.items():
        ex = mr.acc_exact(v)
        recs = [hip.reduce_vector(expo[list(sets).index(name)])[0], prof[order[name], 0]]
        neg = prof[order[name], 1]
        assert (float(neg["n"]), float(neg["shift"]), float(neg["s1"]), float(neg["s2"])) == (n, 0.0, 0.0, 0.0)      # min(x, 0) of x > 0
        for rec in recs:
            s1, s2 = float(rec["s1"]), float(rec["s2"])
            print(f"{name} n={n}: s1 off by {abs(s1 - ex['s1']):.3e} (bound {n * U * ex['abs1']:.3e}), "
                  f"s2 off by {abs(s2 - ex['s2']):.3e} (bound {(n + 3) * U * ex['s2']:.3e})")
            assert float(rec["n"]) == n and float(rec["shift"]) == v[0]
            assert abs(s1 - ex["s1"]) <= n * U * ex["abs1"]
            assert abs(s2 - ex["s2"]) <= (n + 3) * U * ex["s2"]
            val, err = mean_and_error(np.array([n, v[0], s1, s2]))
            m_ref, e_ref, m2_ref = mr.mean_err_longdouble(v)
            assert abs(val - m_ref) <= 1e-8 * abs(m_ref)
            if name == "constant":
                assert s1 == 0.0 and s2 == 0.0 and err == 0.0 and val == v[0]
            elif name == "smooth":
                assert abs(err - e_ref) <= 1e-6 * e_ref
            else:
                # M2 = s2 - s1^2/n.  With |ds1| <= a = n u sum|d| and |ds2| <= b = (n + 3) u sum d^2 :
                #   |dM2| <= b + (2 |s1| a + a^2) / n + 3 u (s2 + s1^2 / n)      (last term: the host's three roundings)
                # and err = sqrt(M2 / (n - 1) / n) is monotone in M2.
                a, b = n * U * ex["abs1"], (n + 3) * U * ex["s2"]
                dm2 = b + (2.0 * abs(ex["s1"]) * a + a * a) / n + 3.0 * U * (ex["s2"] + ex["s1"] ** 2 / n)
                lo = math.sqrt(max(m2_ref - dm2, 0.0) / (n - 1.0) / n) * (1.0 - 4 * U)
                hi = math.sqrt((m2_ref + dm2) / (n - 1.0) / n) * (1.0 + 4 * U)
                print(f"outlier n={n}: err {err:.9e} ref {e_ref:.9e} allowed [{lo:.9e}, {hi:.9e}]")
                assert lo <= err <= hi


@gpu
@pytest.mark.parametrize("n", [1, 257, 4099])
def test_unsecured_bit_equal(n, hip):
    """k4_unsecured, grid (ceil(n / 256), E): one partial block (n = 1), a 1-path tail block (257), 17 blocks (4099); bit-equal to
    unsecured_np on the special-value matrix for the three descriptor kinds"""
    x = special_matrix(n, 50)
    expo = place(hip, x, n + 5)
    for kind, (rows, delayed, h, coll) in descriptors(9, 0.25).items():
        got = hip.unsecured(UnsecuredSpec(rows, delayed, h, coll), expo).cpu().numpy()
        assert bits_equal(got, mr.unsecured_np(x, rows, delayed, h, coll)), kind


# ---- CVA ------------------------------------------------------------------------------------------------------------------------------
# largest relative discrepancy of (mean, error) from the long-double reference below over the path counts of each route, as measured
# on the MI355X (256 CUs, seed 60).  Both kernels sit at the last bit of a double: the scalar kernel's mean equals the reference's
# exactly, so its value assertion is an equality; the table exponentials of the vector kernel cost at most one unit in the last place.
CVA_MEASURED = {"scalar": (0.0, 1.588e-16), "vector": (1.550e-16, 1.589e-16)}
CVA_CAP = (1e-8, 1e-6)


def cva_tolerance(route):
    """4 x the measured discrepancy (the margin covers other seeds), never above the project's rtol"""
    return tuple(min(4.0 * m, c) for m, c in zip(CVA_MEASURED[route], CVA_CAP))


@pytest.fixture(scope="module")
def cva_setup(hip, oracle):
    """book and CVA atoms of irs_cva after prepare(); synthetic paths (uniform within the range each state variable takes on each
    date of a small simulation of the case) and N(0, 0.05) exposures at n_max = (T + 3) * 256 paths, T = 16 * CUs; the per-path
    integrand from the oracle's atoms, combined in long double"""
    sc, _ = cases.make_controller("irs_cva", hip, inject=False)
    sc.run_simulation()                                     # (prepare() + one 1024-path pass, whose paths give the state ranges)
    small = sc.last_state["paths"].cpu().numpy()
    T = 16 * int(hip.device_info()["n_cu"])
    n_max = (T + 3) * 256
    rng = np.random.default_rng(60)
    lo, hi = small.min(axis=2, keepdims=True), small.max(axis=2, keepdims=True)
    paths = lo + (hi - lo) * rng.random(small.shape[:2] + (n_max,))
    rows = sc.metric_exposure_indices.numpy()
    expo = 0.05 * rng.standard_normal((int(sc.book_plan.n_expo_rows), n_max))
    m_i = next(iter(sc._cva_atoms))
    surv, cond = sc._cva_atoms[m_i]
    recovery = sc.risk_metrics.metrics[m_i].recovery_rate
    pt = torch.from_numpy(paths)
    sp = oracle.resolve_atoms(sc.book, surv, pt).numpy().astype(np.longdouble)
    cs = oracle.resolve_atoms(sc.book, cond, pt).numpy().astype(np.longdouble)
    e = np.maximum(expo[rows[:-1]], 0.0).astype(np.longdouble)
    v = ((e * sp * (1 - cs)).sum(axis=0) * (np.longdouble(1.0) - np.longdouble(recovery))).astype(np.float64)
    return dict(sc=sc, T=T, n_max=n_max, unsec=UnsecuredSpec(rows, None, 0.0, False), surv=surv, cond=cond, recovery=recovery,
                paths=hip.from_numpy(paths), expo=hip.from_numpy(expo), poison=hip.from_numpy(np.full_like(expo, np.inf)), v=v, cache={})


def _cva_run(hip, s, n):
    if n not in s["cache"]:
        # the integrands pass through the handle's per-path scratch vector, which an earlier call on the same data leaves holding
        # the right values: overwrite all n_max entries with non-finite ones (infinite exposures), so that a store the kernel under
        # test skips cannot go unnoticed
        hip.reduce_cva(s["sc"].book, s["unsec"], s["surv"], s["cond"], s["recovery"], s["poison"], s["paths"])
        rec = hip.reduce_cva(s["sc"].book, s["unsec"], s["surv"], s["cond"], s["recovery"], s["expo"][:, :n], s["paths"][:, :, :n])[0]
        s["cache"][n] = (rec, mr.acc_exact(s["v"][:n]), mr.mean_err_longdouble(s["v"][:n]))
    return s["cache"][n]


CVA_COUNTS = {
    "scalar": [lambda T: (T - 1) * 256],                       # grid T - 1 < 16 CUs: k4_cva_paths just below the switch
    "vector": [lambda T: T * 256 - 255,                         # == (T - 1) * 256 + 1, grid T: the first launch of k4_cva_paths_v<2>
               lambda T: (T + 1) * 256 - 100,                   # grid T + 1 odd: the last block's second chunk dead, its first partial
               lambda T: (T + 2) * 256 - 100,                   # second chunk partial
               lambda T: (T + 2) * 256],                        # full grid
}


@gpu
@pytest.mark.parametrize("route", ["scalar", "vector"])
def test_cva_kernels_against_long_double_reference(route, hip, cva_setup):
    """mcx_reduce_cva launches k4_cva_paths below ceil(n / 256) = T = 16 * CUs blocks and k4_cva_paths_v<2> (two 256-path chunks per
    block, table exponentials) from there on; the path counts are derived from the device's CU count so that they sit on the switch
    and on every tail of the vector kernel (dead and partial second chunk, odd grid).  The tensors are [:, :n] views of one
    n_max-wide allocation, so the columns past n hold other paths' data.
    Measured relative discrepancy from the reference (mean, error): k4_cva_paths 0 (equal to the last bit), 1.588e-16;
    k4_cva_paths_v<2> 1.550e-16, 1.589e-16.  Asserted: 4 x measured (CVA_MEASURED), far below the cap at the project's 1e-8 / 1e-6.
    Each figure is printed before it is asserted."""
    s = cva_setup
    tol_v, tol_e = cva_tolerance(route)
    for f in CVA_COUNTS[route]:
        n = f(s["T"])
        rec, ex, (m_ref, e_ref, _) = _cva_run(hip, s, n)
        assert float(rec["n"]) == n
        val, err = mean_and_error(np.array([rec["n"], rec["shift"], rec["s1"], rec["s2"]]))
        dv, de = abs(val - m_ref) / abs(m_ref), abs(err - e_ref) / e_ref
        print(f"cva {route} n={n}: value off {dv:.3e}, error off {de:.3e}, shift off {abs(float(rec['shift']) - ex['shift']):.3e}")
        assert dv <= tol_v and de <= tol_e, (route, n, dv, de)


@gpu
def test_cva_scalar_and_vector_kernels_agree(hip, cva_setup):
    """k4_cva_paths on (T - 1) * 256 paths and k4_cva_paths_v<2> on one path more must differ by the extra path's term, up to the
    two kernels' tolerances on the mean (x n, in units of a sum).  Each record holds s1 relative to ITS kernel's value of path 0
    (the shift), so the sums compared are n * shift + s1, formed in long double."""
    s = cva_setup
    n0 = (s["T"] - 1) * 256
    (r0, _, (m0, _, _)), (r1, _, (m1, _, _)) = _cva_run(hip, s, n0), _cva_run(hip, s, n0 + 1)
    L = np.longdouble
    tot0 = L(n0) * L(float(r0["shift"])) + L(float(r0["s1"]))
    tot1 = L(n0 + 1) * L(float(r1["shift"])) + L(float(r1["s1"]))
    tol = cva_tolerance("scalar")[0] * abs(m0) * n0 + cva_tolerance("vector")[0] * abs(m1) * (n0 + 1)
    print(f"cva sums: vector - scalar - extra path = {float(tot1 - tot0 - L(s['v'][n0])):.3e}, allowed {tol:.3e}")
    assert abs(float(tot1 - tot0 - L(s["v"][n0]))) <= tol


# =====================================================================================================================================
# K5 on the GPU: histograms
# =====================================================================================================================================
PATTERNS = ("equal", "0eq1", "1eq2", "distinct", "neighbours")
KINDS = ("plain", "threshold", "collateralised")
COMBOS = [(shift, bits, n_sel, pat, kind) for shift, bits in DIGITS for n_sel in (1, 2, 3, 4) for pat in PATTERNS for kind in KINDS]


def prefix_pattern(ks, pattern, n_sel, shift, bits):
    """[E][n_sel] prefixes from the sorted keys ks [E][n] of the data, cleared below bit shift + bits as the driver holds them
    before that pass.  Far-apart order statistics share few leading bits.  "neighbours": a data key and copies of it with bits
    flipped INSIDE the last digit (bit 0, bit 8) and, for the fourth selection, in the lowest bit of the digit before it: on every
    pass but the last all four share their prefix; on the last pass (0, 9) selections 1 and 2 take the shared shortcut and 3 does
    not."""
    n = ks.shape[1]
    a, b, c, d = ks[:, 0], ks[:, n // 3], ks[:, (2 * n) // 3], ks[:, n - 1]
    h = n // 2
    cols = {"equal": [b, b, b, b], "0eq1": [b, b, c, d], "1eq2": [a, c, c, d], "distinct": [a, b, c, d],
            "neighbours": [ks[:, h], ks[:, h] ^ np.uint64(1), ks[:, h] ^ np.uint64(0x100), ks[:, h] ^ np.uint64(0x200)]}[pattern]
    hi = shift + bits
    keep = np.uint64(0) if hi >= 64 else np.uint64(((1 << 64) - 1) ^ ((1 << hi) - 1))
    return np.ascontiguousarray(np.stack(cols[:n_sel], axis=1) & keep)


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 257, 4099, 262147])
def test_hist_passes_equal_reference(n, hip):
    """k5_hist<false> through select_hist (host prefixes) and select_hist_dev (device prefixes, n_paths < the tensor's width), and
    k5_hist<true> through select_hist_rows on the unsecured values, all equal to hist_np: every digit of _SELECT_DIGITS plus the
    1-bit digits (0, 1) and (63, 1); n_sel 1..4 (4 x 2^11 bins = 32 KiB of LDS); five prefix patterns, of which three make the
    kernel's `shared` shortcut copy selection 0's bins for some selections only; plain, threshold and collateralised + delayed.
    n < 64: idle lanes; 257 / 4099: tail blocks, one block row; 262147: 33 blocks per date at E = 1, the grid cap
    ceil(16 CUs / E) at E = 5, the UN = 4 strided loop with a ragged end.  E = 512 (MCX_MAX_METRIC_DATES) at n = 4099.  The full
    cross product runs at E = 5 for n <= 4099.  The large settings (n = 262147, E = 1, E = 512) take every 17th combination — 17 is
    coprime to 8, 4, 5 and 3, so every digit, n_sel, pattern and descriptor occurs, but not every pairing of them — plus n_sel = 4
    on each of the five 11-bit digits (the 32 KiB launch)."""
    x = special_matrix(n, 70 + n % 83)
    ld = n + 5 + (n & 1)
    expo_w = place(hip, x, ld, wider=3)                     # [7][n + 3]: columns n .. n + 2 are NaN pads
    expo = expo_w[:, :n]
    for E in ([1, 5, 512] if n == 4099 else [1, 5]):
        descs = descriptors(E, 0.25)
        us = {k: mr.unsecured_np(x, *descs[k]) for k in KINDS}
        specs = {k: UnsecuredSpec(*descs[k]) for k in KINDS}
        ks = {k: np.sort(mr.key_np(us[k]), axis=1) for k in KINDS}
        rows_dev = {}
        for k in KINDS:                                     # plain [E][n + 2] rows for k5_hist<true>, two NaN pads each
            r = np.full((E, n + 2), np.nan)
            r[:, :n] = us[k]
            rows_dev[k] = hip.from_numpy(r)
        row_n = hip.from_numpy(np.full(E, n, dtype=np.int64))
        full = E == 5 and n <= 4099
        big4 = [(sh, b, 4, PATTERNS[q % 5], KINDS[q % 3]) for q, (sh, b) in enumerate(DIGITS) if b == 11]
        for shift, bits, n_sel, pat, kind in (COMBOS if full else COMBOS[(n + E) % 17::17] + big4):
            pf = prefix_pattern(ks[kind], pat, n_sel, shift, bits)
            ref = mr.hist_np(us[kind], pf, shift, bits)
            tag = (n, E, shift, bits, n_sel, pat, kind)
            if shift + bits == 64:
                assert (ref.sum(axis=-1) == n).all()
            got = hip.select_hist(specs[kind], expo, n_sel, pf, shift, bits).cpu().numpy()
            assert np.array_equal(got, ref), ("select_hist",) + tag
            pf_dev = hip.from_numpy(pf.view(np.int64))
            out = torch.full((E, n_sel, 1 << bits), -1, dtype=torch.int64, device=hip.device)
            hip.select_hist_dev(specs[kind], expo_w, n_sel, pf_dev, shift, bits, out, n_paths=n)
            assert np.array_equal(out.cpu().numpy(), ref), ("select_hist_dev",) + tag
            out.fill_(-1)
            hip.select_hist_rows(rows_dev[kind], row_n, n_sel, pf_dev, shift, bits, out)
            assert np.array_equal(out.cpu().numpy(), ref), ("select_hist_rows",) + tag


@gpu
@pytest.mark.parametrize("ld", [1, 300, 4099])
def test_hist_rows_respects_row_lengths(ld, hip):
    """k5_hist<true>: row m holds row_n[m] values, row_n in {0, 1, ld / 2, ld, ld + 7} (an entry above ld is clamped to ld); the rest
    of each row is NaN, whose key would be counted by the hi = 64 pass and by the selection whose prefix is the NaN key.  Each
    histogram sums to the matching elements: min(row_n, ld) on the first pass."""
    lens = np.array([0, 1, ld // 2, ld, ld + 7], dtype=np.int64)
    R = len(lens)
    vals = special_matrix(ld, 80)[[0, 2, 3, 5, 1]]
    rows = np.full((R, ld), np.nan)
    for m in range(R):
        rows[m, :min(lens[m], ld)] = vals[m, :min(lens[m], ld)]
    ks = np.sort(mr.key_np(vals), axis=1)
    rows_dev, lens_dev = hip.from_numpy(rows), hip.from_numpy(lens)
    k = 0
    for shift, bits in DIGITS:
        for n_sel in (1, 2, 3, 4):
            pat = PATTERNS[k % 5]
            k += 1
            pf = prefix_pattern(ks, pat, n_sel, shift, bits)
            if n_sel == 4:                                  # the fourth selection looks for the NaN key
                keep = np.uint64(0) if shift + bits >= 64 else np.uint64(((1 << 64) - 1) ^ ((1 << (shift + bits)) - 1))
                pf[:, 3] = mr.key_np(np.array([np.nan]))[0] & keep
            ref = mr.hist_np(vals, pf, shift, bits, row_n=lens)
            if shift + bits == 64:
                assert np.array_equal(ref.sum(axis=-1), np.tile(np.minimum(lens, ld)[:, None], (1, n_sel)))
            out = torch.full((R, n_sel, 1 << bits), -1, dtype=torch.int64, device=hip.device)
            hip.select_hist_rows(rows_dev, lens_dev, n_sel, hip.from_numpy(pf.view(np.int64)), shift, bits, out)
            assert np.array_equal(out.cpu().numpy(), ref), (ld, shift, bits, n_sel, pat)


# ---- k5_narrow ------------------------------------------------------------------------------------------------------------------------
def _narrow_cases(bits):
    """(histogram, rem) pairs: mass in bin 0, in the last bin, in one middle bin, spread with empty bins between; rem at 0, at
    total - 1 and on both sides of every occupied bin's edge"""
    nb = 1 << bits
    shapes = []
    for where in ("first", "last", "middle", "spread"):
        h = np.zeros(nb, dtype=np.int64)
        if where == "first":
            h[0] = 1000
        elif where == "last":
            h[nb - 1] = 1000
        elif where == "middle":
            h[nb // 2] = 1000
        else:
            occ = sorted({0, nb - 1, nb // 2} | set(range(1, nb, max(3, nb // 7))))
            for q, b in enumerate(occ):
                h[b] = 1 + (7 * q) % 5 + (300 if q == 2 else 0)
        shapes.append(h)
    out = []
    for h in shapes:
        tot = int(h.sum())
        edges = np.cumsum(h)[h > 0]
        rems = {0, tot - 1} | {int(e) - 1 for e in edges} | {int(e) for e in edges if e < tot}
        out += [(h, r) for r in sorted(rems)]
    return out


@gpu
@pytest.mark.parametrize("bits", list(range(1, 12)))
def test_narrow_equals_reference(bits, hip):
    """k5_narrow, one block per (date, selection): 2^bits bins over 256 threads (bits <= 8: one bin or none per thread; 9..11: 2, 4, 8
    bins per thread), block scan + reductions.  Hand-built histograms; the new prefix must keep the bits it had and gain the bin at
    `shift`, rem loses the count below the bin.  Launched as n_sel = 4 selections per date and as n_sel = 1."""
    cs = _narrow_cases(bits)
    while len(cs) % 4:
        cs.append(cs[-1])
    hist = np.stack([h for h, _ in cs])
    rem = np.array([r for _, r in cs], dtype=np.int64)
    for shift in sorted({0, 64 - bits, 20}):
        rng = np.random.default_rng(bits * 64 + shift)
        keep = ((1 << 64) - 1) ^ (((1 << bits) - 1) << shift)       # any bits above and below the digit, none in it
        pf = (rng.integers(0, 1 << 63, size=len(cs), dtype=np.uint64) * np.uint64(2) + np.uint64(1)) & np.uint64(keep)
        exp_pf, exp_rem = mr.narrow_np(hist, pf, rem, shift)
        for n_sel in (4, 1):
            d_pf, d_rem = hip.from_numpy(pf.view(np.int64).copy()), hip.from_numpy(rem.copy())
            hip.select_narrow(hip.from_numpy(hist), len(cs) // n_sel, n_sel, shift, bits, d_pf, d_rem)
            assert np.array_equal(d_pf.cpu().numpy().view(np.uint64), exp_pf), (bits, shift, n_sel)
            assert np.array_equal(d_rem.cpu().numpy(), exp_rem), (bits, shift, n_sel)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_six_pass_walk_with_four_selections(kind, hip):
    """k5_hist<false> (n_sel = 4: 32 KiB of LDS on the five 11-bit passes) + k5_narrow over the six digits of _SELECT_DIGITS, device
    resident as the driver runs them: the four order statistics equal those of np.sort by VALUE (special values included): -0.0 == +0.0,
    whose order np.sort leaves open while the key puts -0.0 first, and NaN == NaN, which np.sort puts last, where the key of a
    positive NaN sits.  n = 4099 and 262147, ranks at both ends and two neighbours."""
    for n in (4099, 262147):
        x = special_matrix(n, 90)
        rows, delayed, h, coll = descriptors(5, 0.25)[kind]
        unsec, expo = UnsecuredSpec(rows, delayed, h, coll), place(hip, x, n + 5)
        ranks = [0, n // 3, n // 3 + 1, n - 1]
        prefix = hip.zeros(5, 4, dtype=torch.int64)
        rem = hip.from_numpy(np.tile(np.asarray(ranks, dtype=np.int64), (5, 1)))
        for shift, bits in _SELECT_DIGITS:
            hist = hip.empty(5, 4, 1 << bits, dtype=torch.int64)
            hip.select_hist_dev(unsec, expo, 4, prefix, shift, bits, hist)
            hip.select_narrow(hist, 5, 4, shift, bits, prefix, rem)
        got = mr.key_to_double_np(prefix.cpu().numpy().view(np.uint64))
        assert values_equal(got, np.sort(mr.unsecured_np(x, rows, delayed, h, coll), axis=1)[:, ranks]), n


# =====================================================================================================================================
# K5 on the GPU: the bracket pass, raw outputs
# =====================================================================================================================================
SENTINEL = -7777.0
ROUTES = ("odd_ld", "offset", "collateralised", "vec")


def bracket_values(E, n, inside):
    """u [E][n], lo, hi: date m lives in [1024 (m + 1), 1024 (m + 1) + 40), ranges disjoint over the dates — a candidate written
    to another date's row shows.  Inside values are base + 16 + (i % 1025) / 128: both ends of the bracket [base + 16, base + 24]
    occur.  Every value is a multiple of 2^-7 below 2^13: the shifts of route() are exact."""
    i = np.arange(n)
    u = np.empty((E, n))
    for m in range(E):
        base = 1024.0 * (m + 1)
        ins = inside(i, m)
        low = ((i // 3) % 2 == 0) & ~ins
        u[m] = np.where(ins, base + 16.0 + (i % 1025) / 128.0, np.where(low, base + 1.0 + (i % 7) / 128.0, base + 32.0 + (i % 5) / 128.0))
    base = 1024.0 * (np.arange(E) + 1.0)
    return u, base + 16.0, base + 24.0


def route(hip, u, which, h):
    """(descriptor, exposure view) whose unsecured exposures are exactly u, on the wanted launch of mcx_select_bracket.  VEC needs an
    uncollateralised descriptor, an even ld and a 16-byte aligned base; each of the three other routes breaks one of these.  Dates
    name the matrix rows in reverse order; the last row is named by nobody and is NaN, as are the pad columns.  Threshold h: stored
    x = u + h (all u here are positive or NaN), so that dev_thr returns u; collateralised: e = u + c, delayed row c + h."""
    E, n = u.shape
    assert h == 0.0 or not np.isnan(u).any()
    rev = np.arange(E)[::-1].copy()
    if which == "collateralised":
        c = 8.0 * (np.arange(E)[:, None] + 1.0) + (np.arange(n)[None, :] % 3)
        delayed = np.where(np.arange(E) % 2 == 0, 2 * E - 1 - np.arange(E), -1)          # dates 0, 2, ..: row E + rev
        e = u + np.where((np.arange(E) % 2 == 0)[:, None], c, 0.0)
        mat = np.concatenate([e[rev], (c + h)[rev], np.full((1, n), np.nan)])
        ld = (n + 6) & ~1
        return UnsecuredSpec(rev, delayed, h, True), place(hip, mat, ld)
    mat = np.concatenate([(u + h)[rev], np.full((1, n), np.nan)])
    if which == "odd_ld":
        return UnsecuredSpec(rev, None, h, False), place(hip, mat, (n + 5) | 1)
    ld = (n + 6) & ~1
    return UnsecuredSpec(rev, None, h, False), place(hip, mat, ld, offset=1 if which == "offset" else 0)


def run_bracket(hip, unsec, expo, lo, hi, cap):
    """-> (below [E], raw count [E], candidate buffer [E + 1][cap] whose last row is a spare the kernel must not touch)"""
    E = unsec.n_dates
    buf = torch.full((E + 1, cap), SENTINEL, dtype=torch.float64, device=hip.device)
    counts = torch.full((2, E), -1, dtype=torch.int64, device=hip.device)
    hip.select_bracket(unsec, expo, hip.from_numpy(np.asarray(lo, dtype=np.float64)), hip.from_numpy(np.asarray(hi, dtype=np.float64)),
                       counts, buf[:E])
    c = counts.cpu().numpy()
    return c[0], c[1], buf.cpu().numpy()


def check_complete(out, ref, tag):
    """no LOST bit; below, count and the sorted candidates equal the reference; nothing written past the count or into the spare row"""
    below, raw, buf = out
    for m, (b_ref, inside) in enumerate(ref):
        assert int(below[m]) == b_ref, tag + (m, "below")
        assert int(raw[m]) == len(inside), tag + (m, "count", int(raw[m]) & (LOST - 1), int(raw[m]) >= LOST)
        assert bits_equal(np.sort(buf[m, :len(inside)]), inside), tag + (m, "candidates")
        assert (buf[m, len(inside):] == SENTINEL).all(), tag + (m, "row tail")
    assert (buf[len(ref)] == SENTINEL).all(), tag + ("spare row",)


def _all_routes(hip, u, lo, hi, cap, h, tag, routes=ROUTES):
    ref = mr.bracket_np(u, lo, hi)
    outs = {}
    for r in routes:
        unsec, expo = route(hip, u, r, h)
        outs[r] = run_bracket(hip, unsec, expo, lo, hi, cap)
    return ref, outs


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 16383, 16384, 16385, 65536, 65537])
def test_bracket_sparse_hits(n, hip):
    """every 16th path inside (phase shifted per date): a wave stages at most 16 candidates per iteration, no mid-run flush, no
    loss.  All four launches — k5_bracket<false> by an odd ld, by a base pointer one double off 16-byte alignment, by a
    collateralised descriptor; k5_bracket<true> on the even, aligned, plain matrix — give the reference's below, count and candidate
    multiset.  n < 64 / 64 / 65: one wave with idle lanes, full, plus a second wave's single lane; 16384 = 256 x 64 is one block's
    share (grid 1 -> 2 at 16385); 65536 / 65537: grid 4 -> 5.  Odd n on the even ld is the VEC tail: the last mcx_d2 load is replaced
    by one scalar load."""
    E = 3
    u, lo, hi = bracket_values(E, n, lambda i, m: (i + m) % 16 == 0)
    ref, outs = _all_routes(hip, u, lo, hi, max(n // 8, 64), 0.5, (n,))
    for r, out in outs.items():
        check_complete(out, ref, (n, r))


@gpu
@pytest.mark.parametrize("n", [65536, 65537])
def test_bracket_mid_run_flush(n, hip):
    """k5_bracket<false>, every 5th path inside: each aligned run of 64 paths holds 12 or 13 hits, a wave reads 4 x 64 paths per
    iteration and looks at its stage every K5_FLUSH_EVERY = 8 iterations, so it has staged 384..416 candidates by then — above
    K5_STAGE / 2 = 256 (it flushes mid-run, with its own reservation on the date's counter) and below K5_STAGE = 512 (nothing is
    lost).  n >= 65536: 16 iterations per thread (13 at 65537 on 5 blocks), so the flush happens before the loop ends."""
    i = np.arange(n)
    runs = np.add.reduceat((i % 5 == 0).astype(np.int64), np.arange(0, n - n % 64, 64))
    assert set(runs.tolist()) <= {12, 13}
    u, lo, hi = bracket_values(3, n, lambda i, m: (i + m) % 5 == 0)
    ref, outs = _all_routes(hip, u, lo, hi, n // 4, 0.5, (n,), routes=ROUTES[:3])
    for r, out in outs.items():
        check_complete(out, ref, (n, r))


@gpu
def test_bracket_flat_row_reports_loss(hip):
    """every path inside: each wave stages 2048 (VEC: 4096) candidates between two looks, far above K5_STAGE.  The count stays exact,
    MCX_SELECT_LOST is added, below is 0; the candidate rows hold only values of their own date and the spare row is untouched"""
    n, cap = 65536, 2048
    u, lo, hi = bracket_values(3, n, lambda i, m: i >= 0)
    _, outs = _all_routes(hip, u, lo, hi, cap, 0.5, ("flat",))
    for r, (below, raw, buf) in outs.items():
        for m in range(3):
            assert int(raw[m]) & (LOST - 1) == n and int(raw[m]) >= LOST and int(below[m]) == 0, (r, m, int(raw[m]))
            w = buf[m][buf[m] != SENTINEL]
            assert ((w >= lo[m]) & (w <= hi[m])).all(), (r, m)
        assert (buf[3] == SENTINEL).all(), r


@gpu
def test_bracket_cap_overflow_without_loss(hip):
    """every 16th path inside and cap = 1024 < n / 16 = 4096: no stage overflows, so no LOST bit; count is exact and above cap
    (the caller's sign that the row is incomplete); exactly the cap slots are written, each with a value of the date's inside set,
    none more often than the set holds it"""
    n, cap = 65536, 1024
    u, lo, hi = bracket_values(3, n, lambda i, m: (i + m) % 16 == 0)
    ref, outs = _all_routes(hip, u, lo, hi, cap, 0.5, ("cap",))
    for r, (below, raw, buf) in outs.items():
        for m, (b_ref, inside) in enumerate(ref):
            assert int(below[m]) == b_ref and int(raw[m]) == len(inside) == 4096 and int(raw[m]) > cap, (r, m, int(raw[m]))
            vals, cnt = np.unique(buf[m], return_counts=True)
            ref_vals, ref_cnt = np.unique(inside, return_counts=True)
            assert np.isin(vals, ref_vals).all(), (r, m)
            assert (cnt <= ref_cnt[np.searchsorted(ref_vals, vals)]).all(), (r, m)
        assert (buf[3] == SENTINEL).all(), r


@gpu
def test_bracket_ends(hip):
    """lo = -inf / hi = +inf; lo == hi on a tied value; lo on a value present many times.  below counts strictly less, inside is
    inclusive at both ends, a NaN is neither.  n = 1000 (about 250 paths per wave: below K5_STAGE even with every path inside),
    threshold 0 so that the NaNs reach the comparison; all four launches"""
    n, E = 1000, 4
    rng = np.random.default_rng(100)
    u = np.round(rng.standard_normal((E, n)) * 4.0) / 2.0 + 1024.0 * (np.arange(E)[:, None] + 1.0)      # ties on a 0.5 grid
    u[:, ::37] = np.nan
    tie = 1024.0 * (np.arange(E) + 1.0)                      # the mode of each date: present ~100 times
    assert all((u[m] == tie[m]).sum() > 50 for m in range(E))
    inf = np.full(E, np.inf)
    for name, lo, hi in (("open", -inf, inf), ("point", tie, tie), ("lo_on_tie", tie, tie + 1.0), ("hi_on_tie", tie - 1.5, tie),
                         ("half_open", -inf, tie), ("empty", tie + 0.25, tie + 0.3)):
        ref, outs = _all_routes(hip, u, lo, hi, n, 0.0, (name,))
        assert name != "open" or all(b == 0 and len(ins) == n - len(u[0, ::37]) for b, ins in ref)
        for r, out in outs.items():
            check_complete(out, ref, (name, r))


@gpu
@pytest.mark.parametrize("which", ["collateralised", "odd_ld"])
def test_bracket_driver_takes_every_smooth_row(which, hip):
    """_select_order_stats with bracket_select on, 2^19 + 1 paths and bracket_sample = 4096, for a collateralised descriptor with
    delayed rows and for an odd-ld matrix (both k5_bracket<false>): equal to np.sort, and NO date falls back.  The four dates are
    iid draws from continuous laws — normal, lognormal, uniform, and a normal minus 0.3 x another normal row (the collateral) — so
    the sample's order statistics 5 sigma either side of the rank contain it and the ~2 % of paths inside stay far below the
    candidate cap: bracket_dates == 4 under the driver's own rule (contained, not overflowed, not a point)."""
    from mcx.parallel import Shard
    n, E = (1 << 19) + 1, 4
    rng = np.random.default_rng(110)
    x = rng.standard_normal((E + 2, n))
    x[1] = np.exp(x[1])
    x[2] = rng.random(n) * 10.0 - 5.0
    x[E] *= 0.3
    x[E + 1] = np.nan
    rows = np.array([3, 1, 0, 2])
    if which == "collateralised":
        delayed, h, coll, ld = np.array([E, -1, E, -1]), 0.05, True, n + 5
    else:
        delayed, h, coll, ld = None, 0.05, False, n + 4
        assert ld % 2 == 1
    unsec = UnsecuredSpec(rows, delayed, h, coll)
    sc, _ = cases.make_controller("bs_european", hip, inject=False)
    sc.num_paths_mainsim, sc.bracket_sample, sc.bracket_select = n, 4096, True
    q = int(math.ceil(0.95 * n)) - 1
    ranks = [q - 1, q, q + 1]
    vals = sc._select_order_stats(Shard(), unsec, place(hip, x, ld), ranks)
    assert sc.last_select["bracket_dates"] == E and sc.last_select["fallback_dates"] == 0, sc.last_select
    assert values_equal(vals, np.sort(mr.unsecured_np(x, rows, delayed, h, coll), axis=1)[:, ranks])
