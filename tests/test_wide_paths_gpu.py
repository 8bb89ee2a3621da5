"""Wide models on the GPU: the path kernel for 9 .. 32 correlated one-factor sub-models (csrc/k1_wide.hip, mcx_sim_create_wide).

 1. equality with the narrow route on models both can run (force_wide), bit for bit;
 2. widths the narrow route cannot run, against the numpy restatement tests/wide_paths_reference.py on the normals of
    mcx_rng_draws — which pins the counter layout (path, sub-step, draw = f >> 1, component f & 1) for n_z > 8;
 3. split launches and three emulated ranks;
 4. refusals: every return code of mcx_sim_create_wide, the entry points without a wide form, mcx_book_create's n_state;
 5. end to end against fixtures generated from the reference (tests/golden/gen_wide_golden.py), unfused, and the book results on
    the GPU's own paths against the oracle's book evaluation;
 6. sensitivities of a wide book by bump-and-revalue against the reference's autograd.

Shapes (tests/wide_cases.py): 3 dates of which the first is the calibration date, two distinct gaps, 2 sub-steps per gap; 1 / 255 /
257 paths in a padded tensor.  Bound of (2): four times the restatement's own rounding (float64 run against long-double run,
relative to the largest entry of a row), measured per model on the CPU at the 257 paths that contain the smaller sets."""
import ctypes as C

import numpy as np
import pytest
import torch

import wide_cases as wc
import wide_paths_reference as wr
from mcx import _abi

pytestmark = pytest.mark.gpu
SEED = 43
NAN = float("nan")


def _sim(hip, name, force_wide=False):
    plan = wc.plan_of(name, force_wide=force_wide)
    return plan, plan.create_sim(hip)


def _padded(hip, plan, n):
    """[T][D][n] view of a NaN-filled buffer whose rows are LD_PAD doubles longer"""
    buf = torch.full((plan.n_dates, plan.n_state, n + wc.LD_PAD), NAN, dtype=torch.float64, device=hip.device)
    return buf, buf[:, :, :n]


def _philox(hip, sim, n, offset):
    buf, view = _padded(hip, sim.plan, n)
    hip.generate_paths(sim, SEED, offset, n, out=view)
    hip.synchronize()
    assert torch.isnan(buf[:, :, n:]).all(), "the padding of the leading dimension was written"
    assert not torch.isnan(view).any()
    return view


def _start_states(plan, n, rng):
    """per-path start states around the model's own: every column scaled by a factor in [0.8, 1.2], integrals shifted off zero"""
    st = np.tile(np.asarray(plan.init_state)[:, None], (1, n)) * rng.uniform(0.8, 1.2, size=(plan.n_state, n))
    return np.ascontiguousarray(st + (np.asarray(plan.init_state)[:, None] == 0.0) * rng.uniform(0.0, 0.05, size=(plan.n_state, n)))


# ---- 1. equality with the narrow route ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", wc.N_PATHS)
@pytest.mark.parametrize("name", list(wc.NARROW))
def test_forced_wide_route_equals_the_narrow_route(name, n, hip):
    plan_n, sim_n = _sim(hip, name)
    plan_w, sim_w = _sim(hip, name, force_wide=True)
    assert not plan_n.wide and plan_w.wide
    dn, dw = hip.sim_describe(sim_n), hip.sim_describe(sim_w)
    assert dw == dict(signature="WIDE", n_slots=plan_w.n_slots, n_z=plan_w.n_slots)
    print(f"WIDE-EQ {name} n={n}: the narrow route is {dn['signature']}")
    for offset in (0, 1000):
        a, b = _philox(hip, sim_n, n, offset), _philox(hip, sim_w, n, offset)
        assert torch.equal(a, b), (name, n, offset, dn["signature"], float((a - b).abs().max()))
    rng = np.random.default_rng(7 + n)
    z = hip.from_numpy(rng.standard_normal((plan_n.n_steps, plan_n.n_z, n)))
    a = hip.generate_paths(sim_n, 0, 0, n, inject_z=z)
    b = hip.generate_paths(sim_w, 0, 0, n, inject_z=z)
    assert torch.equal(a, b), (name, n, "injected", dn["signature"])
    st = hip.from_numpy(_start_states(plan_n, n, rng))
    for kw in (dict(inject_z=z), dict()):                      # the per-path start state, with injected and with Philox draws
        a = hip.generate_paths(sim_n, SEED, 17, n, init_state=st, **kw)
        b = hip.generate_paths(sim_w, SEED, 17, n, init_state=st, **kw)
        assert torch.equal(a, b), (name, n, "from state", sorted(kw), dn["signature"])
        assert torch.equal(b[0], st), "the dates before the first sub-step hold the caller's start state"


# ---- 2. widths the narrow route cannot run ------------------------------------------------------------------------------------------
def _device_normals(hip, plan, n, offset):
    """z [n_steps][n_z][n]: normal f of sub-step k is entry f & 1 of draw f >> 1 of mcx_rng_draws"""
    z = np.empty((plan.n_steps, plan.n_z, n))
    for k in range(plan.n_steps):
        for q in range((plan.n_z + 1) // 2):
            _w, _u, zz = hip.rng_draws(SEED, offset, n, k, q)
            zz = zz.cpu().numpy()
            z[k, 2 * q] = zz[0]
            if 2 * q + 1 < plan.n_z:
                z[k, 2 * q + 1] = zz[1]
    return z


_YARDSTICK = {}


def _yardstick(hip, name, plan):
    """(own rounding of the restatement, its long-double paths, the normals) at the largest path count, once per model"""
    if name not in _YARDSTICK:
        n = max(wc.N_PATHS)
        z = _device_normals(hip, plan, n, 0)
        own, hi = wr.own_rounding(plan, z)
        assert hi.min_y > 1e-3 or hi.min_y == np.inf, (name, "a CIR++ path comes near the floor's kink", hi.min_y)
        assert own > 0.0
        _YARDSTICK[name] = (own, hi.paths, z)
    return _YARDSTICK[name]


@pytest.mark.parametrize("n", wc.N_PATHS)
@pytest.mark.parametrize("name", list(wc.WIDE))
def test_wide_paths_against_the_numpy_restatement(name, n, hip):
    plan, sim = _sim(hip, name)
    assert plan.wide and plan.n_z == plan.n_slots > _abi.MAX_SLOTS
    assert hip.sim_describe(sim) == dict(signature="WIDE", n_slots=plan.n_slots, n_z=plan.n_slots)
    own, ref, _z = _yardstick(hip, name, plan)
    got = _philox(hip, sim, n, 0).cpu().numpy()
    gap = wr.row_relative_gap(got, ref[:, :, :n])              # (no path is left out: paths 0 .. n-1 of the 257)
    print(f"WIDE-REF {name} n={n}: restatement's own rounding {own:.3e}, device gap {gap:.3e}, bound {4 * own:.3e}")
    assert gap <= 4.0 * own, (name, n, gap, own)


def test_wide_injected_draws_and_start_states_against_the_restatement(hip):
    """the injected route and the per-path start of a 17-slot model: the same bound, on draws and states of the test's own"""
    name, n = "mix_17_euler", 257
    plan, sim = _sim(hip, name)
    rng = np.random.default_rng(5)
    z, st = rng.standard_normal((plan.n_steps, plan.n_z, n)), _start_states(plan, n, rng)
    own, hi = wr.own_rounding(plan, z, st)
    assert hi.min_y > 1e-3
    got = hip.generate_paths(sim, 0, 0, n, inject_z=hip.from_numpy(z), init_state=hip.from_numpy(st)).cpu().numpy()
    gap = wr.row_relative_gap(got, hi.paths)
    print(f"WIDE-REF injected {name}: own rounding {own:.3e}, device gap {gap:.3e}")
    assert gap <= 4.0 * own, (gap, own)


# ---- 3. split launches, emulated ranks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mix_9_euler", "mix_32_euler", "bs_12_analytical"])
def test_two_launches_split_at_a_path_offset_give_the_bytes_of_one(name, hip):
    plan, sim = _sim(hip, name)
    n, cut, off = 257, 100, 2 ** 33 + 5
    whole = _philox(hip, sim, n, off)
    buf, view = _padded(hip, plan, n)
    hip.generate_paths(sim, SEED, off, cut, out=buf[:, :, :cut])
    hip.generate_paths(sim, SEED, off + cut, n - cut, out=buf[:, :, cut:n])
    hip.synchronize()
    assert torch.equal(view, whole) and torch.isnan(buf[:, :, n:]).all()


def _results(res):
    return [[np.array(m, dtype=float) for m in ns] for ns in res.results]


def test_three_emulated_ranks_match_the_single_shard_run(hip):
    """fixture case (b) — ten correlated factors, three counterparties — on Philox draws with the paths on three ranks"""
    from emulated_ranks import run_ranks
    from mcx import _native
    n_main, n_pre = 6001, 3002

    def build(be):
        sc, _ = wc.make_controller("wide_cva10", be, inject=False, n_main=n_main, n_pre=n_pre)
        sc.materialize = False
        return sc

    ref = _results(build(hip).run_simulation())
    out, calls = run_ranks(3, lambda rank: build(_native.HipBackend(0)), lambda sc, rank: _results(sc.run_simulation()))
    assert calls["all_reduce"] + calls["all_gather"] > 0
    for rank, got in enumerate(out):
        for ns_r, ns_g in zip(ref, got):
            for m_i, (m_r, m_g) in enumerate(zip(ns_r, ns_g)):
                assert np.allclose(m_r[:, 0], m_g[:, 0], rtol=1e-9, atol=1e-12), (rank, m_i, m_r[:, 0], m_g[:, 0])


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def _create_wide(hip, plan, edit=None, slots=None):
    """mcx_sim_create_wide on a copy of the plan's descriptor after edit(desc); -> (return code, sim pointer)"""
    d = _abi.WideSimDesc.from_buffer_copy(plan.desc)
    if slots is not None:
        d.slots = C.cast(slots, C.c_void_p)
    if edit:
        edit(d)
    out = C.c_void_p()
    rc = hip.lib.mcx_sim_create_wide(hip.h, C.byref(d), C.byref(out))
    if rc == 0:
        hip.lib.mcx_sim_destroy(out)
    return rc, out.value


def test_every_return_code_of_sim_create_wide(hip):
    plan = wc.plan_of("mix_9_euler")
    assert _create_wide(hip, plan)[0] == 0
    out = C.c_void_p()
    assert hip.lib.mcx_sim_create_wide(hip.h, None, C.byref(out)) == -1
    assert hip.lib.mcx_sim_create_wide(None, C.byref(plan.desc), C.byref(out)) == -1
    assert hip.lib.mcx_sim_create_wide(hip.h, C.byref(plan.desc), None) == -1

    def field(name, value):
        return lambda d: setattr(d, name, value)

    def slot_copy(i, f, v):
        recs = (_abi.Slot * plan.n_slots).from_buffer_copy(plan.slot_records)
        setattr(recs[i], f, v)
        return recs

    assert _create_wide(hip, plan, field("n_slots", 0)) == (-2, None)
    assert _create_wide(hip, plan, field("n_slots", _abi.WIDE_MAX_SLOTS + 1)) == (-2, None)
    assert _create_wide(hip, plan, field("n_z", plan.n_z - 1)) == (-2, None)
    assert _create_wide(hip, plan, field("n_z", plan.n_z + 1)) == (-2, None)
    for kind in (_abi.MODEL_HESTON, _abi.MODEL_S2F, 0, 99):
        assert _create_wide(hip, plan, slots=slot_copy(3, "kind", kind)) == (-2, None), kind
    assert "MCX_WIDE_MAX_SLOTS" in hip.lib.mcx_last_error(hip.h).decode() or "wide" in hip.lib.mcx_last_error(hip.h).decode()
    assert _create_wide(hip, plan, slots=slot_copy(2, "state_off", 7)) == (-4, None)
    assert "mcx_sim_create_wide: state offsets must be packed" in hip.lib.mcx_last_error(hip.h).decode()
    assert _create_wide(hip, plan, field("n_state", plan.n_state + 1)) == (-4, None)
    def with_step(f, v, **more):
        st = plan.steps.copy()
        st[f][1] = v
        keep.append(st)

        def edit(d):
            d.steps = st.ctypes.data
            for k, x in more.items():
                setattr(d, k, x)
        return edit

    keep = []
    assert _create_wide(hip, plan, with_step("store_idx", plan.n_dates)) == (-5, None)
    assert _create_wide(hip, plan, with_step("chol_idx", -1)) == (-5, None)
    assert _create_wide(hip, plan, with_step("chol_idx", 1)) == (-5, None)                      # beyond n_chol
    chol2 = np.ascontiguousarray(np.concatenate([plan.chol, plan.chol]))                        # a second factor exists, but ...
    assert _create_wide(hip, plan, with_step("chol_idx", 1, n_chol=2, chol=chol2.ctypes.data)) == (-5, None)    # ... EULER uses factor 0
    assert _create_wide(hip, plan, field("scheme", _abi.SCHEME_ANALYTICAL)) == (-6, None)       # CIR++ has no analytical step map
    assert "mcx_sim_create_wide: slot" in hip.lib.mcx_last_error(hip.h).decode() and "has no step map" in hip.lib.mcx_last_error(hip.h).decode()
    # 1 .. 8 slots are accepted: the equality tests use it
    assert _create_wide(hip, wc.plan_of("vas_1_analytical", force_wide=True))[0] == 0
    assert _create_wide(hip, wc.plan_of("mix_8_euler", force_wide=True))[0] == 0


def test_entry_points_without_a_wide_form_refuse_and_write_nothing(hip):
    """mcx_fused_create and the five forward-mode path entry points on a wide sim: MCX_E_NOT_FUSABLE, a message that names the
    limit, outputs untouched"""
    sc, _ = wc.make_controller("wide_cva10", hip, inject=False)
    sc.prepare()
    sim, plan = sc._sim, sc.sim_plan
    assert plan.wide and sc._fused is None and "wide" in hip.not_fusable_reason and "MCX_MAX_SLOTS" in hip.not_fusable_reason
    lib, NP, n = hip.lib, _abi.TANGENT_NP, 64
    sentinel = C.c_void_p(0xDEAD0)
    fd = _abi.FusedDesc()
    assert lib.mcx_fused_create(hip.h, sim.ptr, sc.book.ptr, C.byref(fd), C.byref(sentinel)) == _abi.E_NOT_FUSABLE
    assert sentinel.value == 0xDEAD0 and "MCX_MAX_SLOTS" in lib.mcx_last_error(hip.h).decode()

    def poison(*shape):
        return torch.full(shape, NAN, dtype=torch.float64, device=hip.device)

    def untouched(*ts):
        hip.synchronize()
        return all(bool(torch.isnan(t).all()) for t in ts)

    from mcx.aad import TangentOption
    opts = (TangentOption * 1)()
    cfs, dcfs = poison(1, n), poison(1, NP, n)
    rc = lib.mcx_tangent_european(hip.h, sim.ptr, opts, C.c_int32(1), C.c_int32(1), C.c_uint64(SEED), C.c_uint64(0), C.c_int64(n),
                                  C.c_int64(n), C.c_void_p(cfs.data_ptr()), C.c_void_p(dcfs.data_ptr()), C.c_int64(n), None, None, None)
    assert rc == _abi.E_NOT_FUSABLE and untouched(cfs, dcfs) and "MCX_MAX_SLOTS" in lib.mcx_last_error(hip.h).decode()
    dslot = np.zeros((plan.n_slots, _abi.SLOT_NPARAM, NP))
    dinit, daux = np.zeros((plan.n_state, NP)), np.zeros((plan.n_steps, plan.n_slots, _abi.AUX, NP))
    dchol = np.zeros((len(plan.chol), plan.n_z, plan.n_z, NP))
    paths, dpaths = poison(plan.n_dates, plan.n_state, n), poison(NP, plan.n_dates, plan.n_state, n)
    host = (_abi.ptr(dslot), _abi.ptr(dinit), _abi.ptr(daux))
    tail = (C.c_uint64(SEED), C.c_uint64(0), C.c_int64(n), C.c_void_p(paths.data_ptr()), C.c_void_p(dpaths.data_ptr()), C.c_int64(n))
    rc = lib.mcx_tangent_paths(hip.h, sim.ptr, *host, *tail, None, None)
    assert rc == _abi.E_NOT_FUSABLE and untouched(paths, dpaths) and "MCX_MAX_SLOTS" in lib.mcx_last_error(hip.h).decode()
    for fn in (lib.mcx_tangent_paths_chol, lib.mcx_tangent_paths_s2f):
        rc = fn(hip.h, sim.ptr, *host, _abi.ptr(dchol), SEED, 0, n, paths.data_ptr(), dpaths.data_ptr(), n, None, None)
        assert rc == _abi.E_NOT_FUSABLE and untouched(paths, dpaths) and "MCX_MAX_SLOTS" in lib.mcx_last_error(hip.h).decode()
    rc = lib.mcx_tangent_paths_heston(hip.h, sim.ptr, *host, _abi.ptr(dchol), SEED, 0, n, paths.data_ptr(), dpaths.data_ptr(), n,
                                      None, None, None)
    assert rc == _abi.E_NOT_FUSABLE and untouched(paths, dpaths) and "MCX_MAX_SLOTS" in lib.mcx_last_error(hip.h).decode()


def test_book_create_takes_the_state_width_of_a_wide_model(hip):
    from mcx.plan import BookCompiler, BookPlan
    for n_state, ok in ((17, True), (40, True), (_abi.WIDE_MAX_STATE, True), (_abi.WIDE_MAX_STATE + 1, False)):
        comp = BookCompiler(None, [0.0, 1.0], 3)
        comp.atoms.append((1, n_state - 1, 0.0, 1.0, 0.0, 0.0, 0.0))          # the last state column of date 1
        comp.atom_src.append(None)
        plan = BookPlan(comp, np.zeros(0, dtype=_abi.PRODUCT_DTYPE), 1, 0, 0, True, False, n_state)
        out = C.c_void_p()
        rc = hip.lib.mcx_book_create(hip.h, C.byref(plan.desc), C.byref(out))
        assert (rc == 0) == ok and (ok or rc == -2), (n_state, rc, hip.lib.mcx_last_error(hip.h))
        if rc == 0:
            paths = hip.from_numpy(np.arange(2.0 * n_state * 5).reshape(2, n_state, 5))
            book = type("B", (), dict(ptr=out, plan=plan))()
            got = hip.resolve_atoms(book, [0], paths).cpu().numpy()
            assert np.array_equal(got[0], paths[1, n_state - 1].cpu().numpy())
            hip.lib.mcx_book_destroy(out)


# ---- 5. end to end against the reference's fixtures -----------------------------------------------------------------------------------
def _check_against_golden(sc, res, g, name):
    """the bounds of tests/test_hip_parity.py::_check_against_golden, restated"""
    ours = sc.last_state["paths"].permute(2, 0, 1).cpu().numpy()
    assert np.allclose(ours, g["paths_main"], rtol=1e-11, atol=1e-13), np.abs(ours - g["paths_main"]).max()
    pre = sc.last_state["paths_pre"].permute(2, 0, 1).cpu().numpy()
    assert np.allclose(pre, g["paths_pre"], rtol=1e-11, atol=1e-13)
    n_coeff = 0
    for i in range(len(sc.products)):
        key = f"expo_coeffs_{i}"
        if key in g.files and g[key].size:
            ref_c, our_c = g[key], sc.regression_coeffs[i].numpy()
            scale = np.maximum(np.abs(ref_c).max(), 1e-300)
            assert np.allclose(our_c, ref_c, rtol=1e-6, atol=1e-8 * scale), (name, i, np.abs(our_c - ref_c).max())
            n_coeff += 1
    assert n_coeff == len(sc.products)
    n_ns = len(sc.netting_sets)
    for ns_i in range(n_ns):
        mine = [i for i in range(len(sc.products)) if sc.product_to_netting_set_idx[i] == ns_i]
        ref = sum(g[f"cfs_{i}"] for i in mine)
        assert np.allclose(sc.last_state["cfs"][ns_i].cpu().numpy(), ref, rtol=1e-10, atol=1e-12)
        ref = sum(g[f"exposures_{i}"] for i in mine)
        assert np.allclose(sc.last_state["expo"][ns_i].cpu().numpy(), ref, rtol=1e-8, atol=1e-10)
    for ns_i in range(n_ns):
        for m_i, metric in enumerate(sc.risk_metrics.metrics):
            ref = g[f"result_{ns_i}_{m_i}"]
            ours = np.array([[v, e] for v, e in res.results[ns_i][m_i]], dtype=np.float64)
            assert np.allclose(ours[:, 0], ref[:, 0], rtol=1e-8, atol=1e-10), (name, metric.get_name(), ours[:, 0], ref[:, 0])
            assert np.allclose(ours[:, 1], ref[:, 1], rtol=1e-6, atol=1e-12), (name, metric.get_name(), ours[:, 1], ref[:, 1])


ORACLE_TOL = 1e-12            # tests/test_book_kernels.py: GPU book results against the oracle's, relative to the largest magnitude of the row


@pytest.mark.parametrize("name", ["wide_basket12_analytical", "wide_basket12_euler", "wide_cva10"])
def test_wide_books_against_the_reference(name, hip, oracle):
    import book_reference as R
    sc, g = wc.make_controller(name, hip, fused=True)
    res = sc.run_simulation()
    assert sc.sim_plan.wide and sc.sim_plan.n_slots > _abi.MAX_SLOTS
    assert sc.allow_fused and sc._fused is None and "wide" in hip.not_fusable_reason      # the unfused route, by the library's refusal
    _check_against_golden(sc, res, g, name)
    if name == "wide_cva10":                     # a CVA metric of another counterparty's netting set is zero, its own is not
        for ns_i in range(3):
            for j in range(3):
                v = res.results[ns_i][2 + j][0][0]
                assert (v > 0.0) if j == ns_i else (v == 0.0), (ns_i, j, v)
    # the book on the GPU's own paths against the oracle's book evaluation (which takes n_state as an argument)
    plan = sc.book.plan
    plan.coeffs[:] = hip.book_get_coeffs(sc.book)
    paths = sc.last_state["paths"].cpu().contiguous()
    ocfs, oexpo = oracle.eval_book(oracle.book_create(plan), paths)
    ref = R.evaluate(plan, paths.numpy())
    cfs, expo = sc.last_state["cfs"].cpu().numpy(), sc.last_state["expo"].cpu().numpy()
    lim = ORACLE_TOL * np.asarray(ref.cfs_M.max(axis=1), dtype=np.float64)[:, None]
    assert (np.abs(cfs - ocfs.numpy()) <= lim).all(), (name, "cashflows differ from the oracle's")
    lim = ORACLE_TOL * np.asarray(ref.expo_M.max(axis=2), dtype=np.float64)[:, :, None]
    assert (np.abs(expo - oexpo.numpy()) <= lim).all(), (name, "exposures differ from the oracle's")


def test_single_step_of_a_wide_model_config(hip):
    """Model.simulate_time_step_euler on a 10-model ModelConfig: the single-step plan through mcx_generate_paths_from_state"""
    from mcx.common.enums import SimulationScheme
    from mcx.plan import SimPlan
    _ns, model, _rm = wc.cva10(wc.mcx_classes())
    n = 255
    rng = np.random.default_rng(3)
    plan = SimPlan.single_step(model, SimulationScheme.EULER, 0.3, 0.55)
    assert plan.wide
    st, w = _start_states(plan, n, rng), rng.standard_normal((1, plan.n_z, n))
    t1, t2 = torch.tensor([0.3], dtype=torch.float64), torch.tensor([0.55], dtype=torch.float64)
    got = model.simulate_time_step_euler(t1, t2, torch.from_numpy(st.T.copy()), torch.from_numpy(w[0].T.copy()))
    own, hi = wr.own_rounding(plan, w, st)
    assert got.shape == (n, plan.n_state)
    gap = wr.row_relative_gap(got.cpu().numpy().T[None], hi.paths)
    assert gap <= 4.0 * own, (gap, own)


# ---- 6. sensitivities ---------------------------------------------------------------------------------------------------------------
def test_wide_book_sensitivities_by_bumps_against_the_reference_autograd(hip):
    """12-asset basket under ANALYTICAL, differentiate=True: no tangent form for a wide model, hence 2 * 25 bumped passes; the
    gradients of PV against the reference's autograd on the recorded draws, under the bounds of check_lsm_sensitivities
    (tests/test_oracle_golden.py), restated for the PV metric"""
    sc, g = wc.make_controller("wide_basket12_analytical_aad", hip)
    res = sc.run_simulation()
    assert sc.timings["tangent"] is False and sc.timings["bumped_passes"] == 2 * 25
    assert list(res.model_param_names) == list(g["param_names"]) and len(g["param_names"]) == 25
    m_i = [m.get_name() for m in sc.risk_metrics.metrics].index("pv")
    ref_v = g[f"result_0_{m_i}"]
    ours_v = np.array(res.results[0][m_i], dtype=np.float64)
    assert np.allclose(ours_v[:, 0], ref_v[:, 0], rtol=1e-8, atol=1e-10)
    ref = g[f"grad_0_{m_i}"]
    ours = np.array(res.derivatives[0][m_i], dtype=np.float64)
    assert ours.shape == ref.shape and not np.isnan(ref).any()
    scale = np.max(np.abs(ref), axis=1, keepdims=True)
    err = np.abs(ours - ref)
    tol = 2e-6 * np.maximum(np.abs(ref), 1e-3 * np.broadcast_to(scale, ref.shape)) + 1e-10
    print("WIDE-AAD worst |bump - autograd| / tol:", float((err / tol).max()))
    assert np.all(err <= tol), (ours, ref)
