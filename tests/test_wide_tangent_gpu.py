"""Forward-mode sensitivities of wide models on the GPU: the per-slot dual path kernel (csrc/kt_wide.hip kt_paths_wide behind
mcx_tangent_paths_wide) and the route through it (mcx.aad.wide_route, SimulationController.tangent_wide).

 1. the kernel against the numpy restatement with explicit tangents (tests/wide_tangent_reference.py) on the normals of mcx_rng_draws
    and on injected normals: every parameter in chunks of 4 in parameter order — the chunk of slot 0, of the last slot at an even
    (16) and an odd (31) row, chunks that straddle two slots, the BlackScholesMulti rate chunk with every slot active, the
    zero-padded last chunk, all-zero tables.  In every launch: the value image is HipBackend.generate_paths' bytes, the tangent
    columns of inactive slots are exactly 0.0, n_active is the count derived from the tables;
 2. the narrow kernels on the same models forced wide, under the same bound;
 3. two launches split at a path offset give the bytes of one;
 4. refusals by code, with nothing written; the narrow entries still refuse the wide sim;
 5. end to end: the 12-asset basket and the ten-factor CVA book with y0 = theta (tests/wide_aad_cases.py) against the reference's
    autograd, the CVA book on three emulated ranks, a 5-slot book forced wide against its own bump route, a book with a Hull-White slot.

Bound of (1) and (2): four times the restatement's own rounding of the tangent images (float64 run against long-double run,
relative to the largest entry of a row, floored at n_sub_steps x 2.2e-16), computed at run time per model, chunk and path count
(on the first n of the 257 paths: a gap on n paths is relative to the rows' largest entries among them, and so is its yardstick).
Measured on the MI355X: yardstick 8.8e-16 (the floor) for the ANALYTICAL models, 1.6e-15 .. 2.2e-15 for the EULER mixes at 257 paths;
worst device gap over all path counts 9.5e-16 .. 4.8e-15 in ten of the twelve cases; 5.6e-12 (17-slot mix, injected), 4.5e-13 and
6.2e-14 (32-slot mix) where a tangent row of few paths is a small residual (d Lambda / d kappa of CIR++ started at y0 = theta), each
inside 4 times the yardstick of its own paths.  Narrow cross-check: mutual gap 0."""
import ctypes as C

import numpy as np
import pytest
import torch

import wide_cases as wc
import wide_tangent_reference as wt
from mcx import _abi, aad
from mcx._native import McxError

pytestmark = pytest.mark.gpu
NP = _abi.TANGENT_NP
SEED = 43
NAN = float("nan")
# EULER mixes cycling V B C D (no Hull-White), and the two BlackScholesMulti widths of tests/wide_cases.py under ANALYTICAL
MODELS = {
    "vbcd_5_euler": (lambda: wc.mixed_model("".join("VBCD"[k % 4] for k in range(5)), 41), "EULER"),
    "vbcd_9_euler": (lambda: wc.mixed_model("".join("VBCD"[k % 4] for k in range(9)), 42), "EULER"),
    "vbcd_17_euler": (lambda: wc.mixed_model("".join("VBCD"[k % 4] for k in range(17)), 43), "EULER"),
    "vbcd_32_euler": (lambda: wc.mixed_model("".join("VBCD"[k % 4] for k in range(32)), 44), "EULER"),
    "bs_12_analytical": (lambda: wc.bs_multi(12, 25), "ANALYTICAL"),
    "bs_32_analytical": (lambda: wc.bs_multi(32, 26), "ANALYTICAL"),
}
_CACHE = {}


def _setup(hip, name, build=None, scheme=None, force_wide=True):
    """(model, plan, sim, derivative tables) once per model; force_wide: the wide sim (a no-op above 8 slots)"""
    from mcx.common.enums import SimulationScheme
    from mcx.plan import SimPlan
    key = (name, force_wide)
    if key not in _CACHE:
        if build is None:
            build, scheme = MODELS[name]
        model = build()
        plan = SimPlan(model, wc.TIMELINE, SimulationScheme[scheme], wc.NUM_STEPS, force_wide=force_wide)
        _CACHE[key] = (model, plan, plan.create_sim(hip), wt.derivative_tables(model, plan))
    return _CACHE[key]


def _device_normals(hip, plan, n, offset=0):
    z = np.empty((plan.n_steps, plan.n_z, n))
    for k in range(plan.n_steps):
        for q in range((plan.n_z + 1) // 2):
            zz = hip.rng_draws(SEED, offset, n, k, q)[2].cpu().numpy()
            z[k, 2 * q] = zz[0]
            if 2 * q + 1 < plan.n_z:
                z[k, 2 * q + 1] = zz[1]
    return z


def _padded(hip, plan, n):
    """NaN-filled (paths, dpaths) buffers whose rows are LD_PAD doubles longer, and their [.., :n] views"""
    p = torch.full((plan.n_dates, plan.n_state, n + wc.LD_PAD), NAN, dtype=torch.float64, device=hip.device)
    d = torch.full((NP, plan.n_dates, plan.n_state, n + wc.LD_PAD), NAN, dtype=torch.float64, device=hip.device)
    return (p, d), (p[:, :, :n], d[:, :, :, :n])


def _launch(hip, sim, d, n, offset=0, inject_z=None):
    """one call into padded buffers -> (paths, dpaths, n_active) with the padding checked"""
    plan = sim.plan
    bufs, views = _padded(hip, plan, n)
    if inject_z is not None:                       # injected draws are read with the leading dimension of the paths
        zb = torch.zeros((plan.n_steps, plan.n_z, n + wc.LD_PAD), dtype=torch.float64, device=hip.device)
        zb[:, :, :n] = inject_z
        inject_z = zb
    _p, _d, n_active = hip.tangent_paths_wide(sim, d["slots"], d["init"], d["aux"], d["chol"], SEED, offset, n, inject_z, out=views,
                                              ld=n + wc.LD_PAD)
    hip.synchronize()
    assert torch.isnan(bufs[0][:, :, n:]).all() and torch.isnan(bufs[1][:, :, :, n:]).all(), "the padding was written"
    return views[0], views[1], n_active


def _column_slots(plan):
    """state column -> slot"""
    out = []
    for r, sl in enumerate(wt.wr.slot_records(plan)):
        out += [r] * wt.wr.STATE_DIM[sl["kind"]]
    return np.array(out)


def _check_chunk(hip, name, plan, sim, sel, d, n, z, ref_hi, own_case, inject):
    """the assertions of one launch; own_case: the yardstick of the case (all 257 paths) -> (device gap on the scale of the case's
    rows, device gap on the scale of the n paths' own rows, n_active)"""
    if inject:
        paths, dpaths, n_active = _launch(hip, sim, d, n, inject_z=hip.from_numpy(z[:, :, :n]))
        primal = hip.generate_paths(sim, 0, 0, n, inject_z=hip.from_numpy(np.ascontiguousarray(z[:, :, :n])))
    else:
        paths, dpaths, n_active = _launch(hip, sim, d, n)
        primal = hip.generate_paths(sim, SEED, 0, n)
    assert torch.equal(paths, primal), (name, sel, n, "the value image is not the path kernel's")
    active = wt.active_from_tables(plan, d["slots"], d["init"], d["aux"], d["chol"])
    assert n_active == len(active) and active == aad.active_slots(plan, d["slots"], d["init"], d["aux"], d["chol"]), (name, sel)
    got = dpaths.cpu().numpy()
    off = ~np.isin(_column_slots(plan), active)
    assert not np.isnan(got).any() and not got[:, :, off].any(), (name, sel, "tangent columns of inactive slots must be exactly 0.0")
    assert not got[len(sel):].any(), (name, sel, "the padding of the last chunk: zero in, zero out")
    # (no path is left out: paths 0 .. n-1 of the 257.)  Two bounds.  Relative to the largest entry of the CASE's rows, the yardstick
    # of the case.  And relative to the largest entry among the n paths themselves — on few paths a tangent row can be a small residual
    # of cancelling terms (d Lambda / d kappa of CIR++ started at y0 = theta), where the restatement's own float64 run loses the same
    # digits — the yardstick of those n paths.  At n = 257 the two coincide.
    gap_case = wt.row_relative_gap(got, ref_hi.dpaths[:, :, :, :n], scale_from=ref_hi.dpaths)
    assert gap_case <= 4.0 * own_case, (name, sel, n, gap_case, own_case)
    own_n = wt.yardstick(ref_hi.lo, ref_hi, n, plan.n_steps)
    gap_n = wt.row_relative_gap(got, ref_hi.dpaths[:, :, :, :n])
    assert gap_n <= 4.0 * own_n, (name, sel, n, gap_n, own_n)
    return gap_case, gap_n, n_active


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inject", [False, True], ids=["philox", "injected"])
@pytest.mark.parametrize("name", list(MODELS))
def test_kernel_against_the_restatement_with_explicit_tangents(name, inject, hip):
    model, plan, sim, dd = _setup(hip, name)
    assert plan.wide and hip.sim_describe(sim)["signature"] == "WIDE"
    P, ns = len(model.get_model_params()), plan.n_slots
    n_max = max(wc.N_PATHS)
    z = np.random.default_rng(17).standard_normal((plan.n_steps, plan.n_z, n_max)) if inject else _device_normals(hip, plan, n_max)
    seen, worst_own, worst_gap, worst_gap_n = [], 0.0, 0.0, 0.0
    for sel, d in wt.chunks(dd, P, NP):
        own, hi = wt.own_rounding(plan, z, d["slots"], d["init"], d["aux"], d["chol"])
        assert hi.min_floor_gap > 1e-3, (name, sel, "a CIR++ path comes near its floor or 0", hi.min_floor_gap)
        for n in wc.N_PATHS:
            gap, gap_n, n_active = _check_chunk(hip, name, plan, sim, sel, d, n, z, hi, own, inject)
            worst_gap, worst_gap_n = max(worst_gap, gap), max(worst_gap_n, gap_n)
        worst_own = max(worst_own, own)
        seen.append((tuple(sel), tuple(wt.active_from_tables(plan, d["slots"], d["init"], d["aux"], d["chol"]))))
    print(f"WIDE-TANGENT {name} {'injected' if inject else 'philox'}: {len(seen)} chunks, largest yardstick {worst_own:.3e}, "
          f"worst device gap {worst_gap:.3e} (on the scale of the launch's own paths {worst_gap_n:.3e}); active slots per chunk {[a for _s, a in seen]}")
    acts = [a for _s, a in seen]
    assert any(a and a[0] == 0 for a in acts), "the chunk of slot 0 (zc = z[0])"
    assert any(ns - 1 in a for a in acts), "the chunk of the last slot"
    assert [len(s) for s, _a in seen] == [NP] * (P // NP) + [P % NP] * (P % NP > 0), "chunks of NP in parameter order"
    if name.endswith("analytical"):
        assert tuple(range(ns)) in acts, "the BlackScholesMulti rate chunk: every slot is active"
        assert len(seen[-1][0]) < NP, "the zero-padded last chunk"
    else:
        assert any(len(a) >= 2 for a in acts), "a chunk that straddles two slots"
    if name == "vbcd_17_euler":
        assert acts[-1] == (16,), "the last slot alone, at an even row"
    if name == "vbcd_32_euler":
        assert acts[-1] == (31,), "the last slot alone, at an odd row"


def test_all_zero_tables_launch_nothing(hip):
    for name in ("vbcd_9_euler", "bs_12_analytical"):
        _model, plan, sim, dd = _setup(hip, name)
        d = {k: np.zeros(v.shape[:-1] + (NP,)) for k, v in dd.items()}
        d.setdefault("chol", None)
        for n in wc.N_PATHS:
            paths, dpaths, n_active = _launch(hip, sim, d, n)
            assert n_active == 0 and not dpaths.cpu().numpy().any()
            assert torch.equal(paths, hip.generate_paths(sim, SEED, 0, n))


# ---- 2. the narrow kernels under the same bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vas_cir_2_euler", "bs_4_analytical"])
def test_narrow_cross_check(name, hip):
    build, scheme = wc.NARROW[name]
    model, plan_w, sim_w, dd = _setup(hip, name, build, scheme, force_wide=True)
    _m, plan_n, sim_n, _dd = _setup(hip, name, build, scheme, force_wide=False)
    assert plan_w.wide and not plan_n.wide
    n, P = 257, len(model.get_model_params())
    z = np.random.default_rng(3).standard_normal((plan_w.n_steps, plan_w.n_z, n))
    d_z = hip.from_numpy(z)
    mutual = 0.0
    for sel, d in wt.chunks(dd, P, NP):
        own, hi = wt.own_rounding(plan_w, z, d["slots"], d["init"], d["aux"], d["chol"])
        assert hi.min_floor_gap > 1e-3
        _p, dw, _n = hip.tangent_paths_wide(sim_w, d["slots"], d["init"], d["aux"], d["chol"], 0, 0, n, d_z)
        if scheme == "ANALYTICAL":
            _p, dn = hip.tangent_paths_chol(sim_n, d["slots"], d["init"], d["aux"], d["chol"], 0, 0, n, d_z)
        else:
            _p, dn = hip.tangent_paths(sim_n, d["slots"], d["init"], d["aux"], 0, 0, n, d_z)
        dw, dn = dw.cpu().numpy(), dn.cpu().numpy()
        g_w, g_n = wt.row_relative_gap(dw, hi.dpaths), wt.row_relative_gap(dn, hi.dpaths)
        scale = np.abs(dn).max(axis=-1, keepdims=True)
        mutual = max(mutual, float((np.abs(dw - dn) / np.where(scale == 0, 1.0, scale)).max()))
        print(f"WIDE-TANGENT narrow {name} {sel}: yardstick {own:.3e}, wide entry {g_w:.3e}, narrow entry {g_n:.3e}")
        assert g_w <= 4.0 * own and g_n <= 4.0 * own, (name, sel, g_w, g_n, own)
    print(f"WIDE-TANGENT narrow {name}: mutual gap of the two entries, relative to a row's largest entry: {mutual:.3e}"
          + (" (identical)" if mutual == 0.0 else ""))


# ---- 3. split launches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [5, 2 ** 33 + 5])
@pytest.mark.parametrize("name", ["vbcd_17_euler", "bs_12_analytical"])
def test_two_launches_split_at_a_path_offset_give_the_bytes_of_one(name, off, hip):
    model, plan, sim, dd = _setup(hip, name)
    n, cut = 257, 100
    sel, d = list(wt.chunks(dd, len(model.get_model_params()), NP))[1 if name.startswith("vbcd") else 0]
    call = lambda o, m, out, z=None: hip.tangent_paths_wide(sim, d["slots"], d["init"], d["aux"], d["chol"], SEED, o, m, z, out=out,
                                                            ld=n + wc.LD_PAD)
    z = torch.zeros((plan.n_steps, plan.n_z, n + wc.LD_PAD), dtype=torch.float64, device=hip.device)
    z[:, :, :n] = hip.from_numpy(np.random.default_rng(9).standard_normal((plan.n_steps, plan.n_z, n)))
    for inject in (False, True):
        (bp, bd), whole = _padded(hip, plan, n)
        call(off, n, whole, z if inject else None)
        (sp, sd), _v = _padded(hip, plan, n)
        call(off, cut, (sp[:, :, :cut], sd[:, :, :, :cut]), z if inject else None)
        call(off + cut, n - cut, (sp[:, :, cut:n], sd[:, :, :, cut:n]), z[:, :, cut:] if inject else None)
        hip.synchronize()
        assert torch.equal(sp[:, :, :n], bp[:, :, :n]) and torch.equal(sd[:, :, :, :n], bd[:, :, :, :n]), (name, off, inject)
        assert torch.isnan(sp[:, :, n:]).all() and torch.isnan(sd[:, :, :, n:]).all()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def _raw_call(hip, sim, plan, n, ld=None, dchol="zeros", paths=None, dpaths=None):
    dslot, dinit = np.zeros((plan.n_slots, _abi.SLOT_NPARAM, NP)), np.zeros((plan.n_state, NP))
    daux = np.zeros((plan.n_steps, plan.n_slots, _abi.AUX, NP))
    dslot[0, 1, 0] = 1.0                                    # an active slot: an accepted call would launch
    dc = np.zeros((max(len(plan.chol), 1), plan.n_z, plan.n_z, NP)) if dchol == "zeros" else None
    return hip.lib.mcx_tangent_paths_wide(hip.h, sim.ptr, _abi.ptr(dslot), _abi.ptr(dinit), _abi.ptr(daux), _abi.ptr(dc) if dc is not None else None,
                                          SEED, 0, n, paths.data_ptr(), dpaths.data_ptr(), n if ld is None else ld, None, None, None)


def test_refusals_write_nothing(hip):
    from mcx.common.enums import SimulationScheme
    from mcx.plan import SimPlan
    n = 64
    E, A, Q = SimulationScheme.EULER, SimulationScheme.ANALYTICAL, SimulationScheme.QE

    def poisoned(plan):
        return (torch.full((plan.n_dates, plan.n_state, n), NAN, dtype=torch.float64, device=hip.device),
                torch.full((NP, plan.n_dates, plan.n_state, n), NAN, dtype=torch.float64, device=hip.device))

    def refused(plan, code, word=None, scheme=None, **kw):
        sim = plan.create_sim(hip)
        if scheme is not None:                     # a scheme no plan of a ModelConfig has: the descriptor edited, as the library sees it
            desc, out = _abi.WideSimDesc.from_buffer_copy(plan.desc), C.c_void_p()
            desc.scheme = scheme
            assert hip.lib.mcx_sim_create_wide(hip.h, C.byref(desc), C.byref(out)) == 0
            sim = type(sim)(out, hip.lib.mcx_sim_destroy, plan)
        p, d = poisoned(plan)
        rc = _raw_call(hip, sim, plan, n, paths=p, dpaths=d, **kw)
        hip.synchronize()
        assert rc == code, (rc, code, hip.lib.mcx_last_error(hip.h))
        assert torch.isnan(p).all() and torch.isnan(d).all(), "a refused call wrote"
        if word:
            assert word in hip.lib.mcx_last_error(hip.h).decode(), hip.lib.mcx_last_error(hip.h)

    refused(wc.plan_of("vas_cir_2_euler"), _abi.E_NOT_FUSABLE, "narrow")                                   # a narrow sim
    refused(wc.plan_of("mix_9_euler"), _abi.E_NOT_FUSABLE, "no tangent step")                              # a Hull-White slot
    refused(SimPlan(wc.mixed_model("D" * 9, 5), wc.TIMELINE, E, wc.NUM_STEPS), _abi.E_NOT_FUSABLE, "scheme", scheme=Q.value)   # QE
    # ANALYTICAL with a slot other than Black-Scholes / Vasicek (deterministic CIR++ runs under every scheme)
    refused(SimPlan(wc.mixed_model("D" * 9, 5), wc.TIMELINE, E, wc.NUM_STEPS), _abi.E_NOT_FUSABLE, "analytic tangent step", scheme=A.value)
    refused(wc.plan_of("bs_12_analytical"), -1, dchol=None)                                                # ANALYTICAL without h_dchol
    refused(wc.plan_of("bs_12_analytical"), -2, "ld < n_paths", ld=n - 1)
    plan = SimPlan(wc.mixed_model("VBCD" * 3, 7), wc.TIMELINE, E, wc.NUM_STEPS)
    refused(plan, -2, "ld < n_paths", ld=n - 1)
    sim = plan.create_sim(hip)
    p, d = poisoned(plan)
    assert _raw_call(hip, sim, plan, n, paths=p, dpaths=d, dchol=None) == 0                                # EULER needs no h_dchol
    hip.synchronize()
    assert not torch.isnan(p).any() and not torch.isnan(d).any()
    # the narrow entries still refuse the wide sim
    dd = {k: np.zeros(s) for k, s in (("slots", (plan.n_slots, _abi.SLOT_NPARAM, NP)), ("init", (plan.n_state, NP)),
                                      ("aux", (plan.n_steps, plan.n_slots, _abi.AUX, NP)))}
    for call in (lambda: hip.tangent_paths(sim, dd["slots"], dd["init"], dd["aux"], SEED, 0, n),
                 lambda: hip.tangent_paths_chol(sim, dd["slots"], dd["init"], dd["aux"], None, SEED, 0, n)):
        with pytest.raises(McxError, match="MCX_MAX_SLOTS") as e:
            call()
        assert e.value.code == _abi.E_NOT_FUSABLE


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------
def test_basket12_forward_mode_against_the_reference_autograd(hip):
    """the fixture of the bump route (tests/test_wide_paths_gpu.py), now in forward mode: 25 parameters in 7 passes"""
    from test_oracle_golden import check_lsm_sensitivities
    sc, g = wc.make_controller("wide_basket12_analytical_aad", hip)
    sc.tangent_wide = True
    assert aad.wide_route(sc)
    res = sc.run_simulation()
    assert sc.timings["tangent"] is True and sc.timings["forward_mode_passes"] == 7 and "bumped_passes" not in sc.timings
    act = sc.timings["wide_active_slots"]                 # the shared rate reaches every asset; a spot or a volatility its own
    assert len(act) == 7 and sorted(act)[-1] == 12 and sorted(act)[-2] <= 4 and min(act) >= 1, act
    assert list(res.model_param_names) == list(g["param_names"])
    m_i = [m.get_name() for m in sc.risk_metrics.metrics].index("pv")
    ref, ours = g[f"grad_0_{m_i}"], np.array(res.derivatives[0][m_i], dtype=np.float64)
    scale = np.abs(ref).max(axis=1, keepdims=True)
    print(f"WIDE-TANGENT basket12 PV: worst |forward - autograd| / row's largest entry = {float((np.abs(ours - ref) / scale).max()):.3e}")
    # check_lsm_sensitivities on the PV rows (the fixture holds the reference's gradients of PV): one netting set, one metric
    pv = {"param_names": g["param_names"], "result_0_0": g[f"result_0_{m_i}"], "grad_0_0": ref}
    only_pv = type("R", (), dict(model_param_names=res.model_param_names, results=[[res.results[0][m_i]]],
                                 derivatives=[[res.derivatives[0][m_i]]]))()
    check_lsm_sensitivities(sc, pv, only_pv)


def _five_slot_book(hip, tangent_wide, letters="BBVCD", seed=12):
    """a European call on the first asset plus a payer swap on the short rate; PV and EPE"""
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    mod = wc.mcx_classes()
    model = wc.mixed_model(letters, seed, mod)
    rates = next(f"ir{k}" for k, c in enumerate(letters) if c == "V")
    call = mod["EuropeanOption"](mod["Equity"]("eq0"), 1.0, 85.0, mod["OptionType"].CALL, asset_id="eq0")
    call.name = "call"
    swap = mod["InterestRateSwap"](0.0, 1.0, 1.0, 0.03, 0.5, 0.5, mod["IRSType"].PAYER, rates)
    swap.name = "swap"
    ns = [mod["NettingSet"](name="book", products=[call, swap])]
    rm = mod["RiskMetrics"]([mod["PVMetric"](), mod["EPEMetric"]()], exposure_timeline=np.array([0.0, 0.5, 1.0]))
    sc = SimulationController(ns, model, rm, 4096, 2048, 2, SimulationScheme.EULER, differentiate=True, backend=hip)
    sc.tangent_wide = tangent_wide
    return sc


def test_five_slot_book_forced_wide_agrees_with_its_bump_route(hip):
    """a narrow model the narrow dual kernels have no instantiation for: with the flag the pass forces the plan wide; without it the
    book is bumped as before.  Bound of the comparison: the bump's own truncation, 4e-6 of the row (tests/test_tangent_heston_gpu.py)"""
    fwd, bump = _five_slot_book(hip, True), _five_slot_book(hip, False)
    assert aad.wide_route(fwd) and not aad.wide_route(bump)
    # the forward controller keeps the default allow_fused = True: its base pass runs on a forced-wide plan, which the fused pass
    # refuses at creation, so the book runs unfused.  The NARROW 5-slot semi-fused evaluation (mcx_fused_eval_paths) has no
    # instantiation for 5 slots and raises instead of falling back — with or without this route — so the bumped controllers run unfused
    assert fwd.allow_fused is True
    bump.allow_fused = False
    g_f, g_b = fwd.run_simulation().derivatives, bump.run_simulation().derivatives
    P = len(fwd.model.get_model_params())
    assert fwd.timings["tangent"] is True and fwd.timings["forward_mode_passes"] == (P + NP - 1) // NP and fwd.sim_plan.wide
    assert bump.timings["tangent"] is False and bump.timings["bumped_passes"] == 2 * P and not bump.sim_plan.wide
    for m_i in range(len(g_f[0])):
        a, b = np.array(g_f[0][m_i], dtype=np.float64), np.array(g_b[0][m_i], dtype=np.float64)
        scale = np.abs(b).max(axis=1, keepdims=True)
        gap = np.abs(a - b) / np.where(scale == 0, 1.0, scale)
        print(f"WIDE-TANGENT five slots, metric {m_i}: forward against bumped, worst gap / row's largest entry = {gap.max():.3e}")
        assert np.all(gap <= 4e-6), (m_i, gap.max())


def _grads(res):
    return [[np.array(m, dtype=np.float64) for m in per_ns] for per_ns in res.derivatives]


def test_cva10_forward_mode_against_the_reference_autograd(hip):
    """the ten-factor CVA book with y0 = theta (tests/wide_aad_cases.py): a Vasicek short rate and nine CIR++ hazard models, three
    netting sets, PV, EPE and one CVA per counterparty — every row under check_lsm_sensitivities"""
    import wide_aad_cases as wa
    from test_oracle_golden import check_lsm_sensitivities
    sc, g = wa.make_controller("wide_cva10_aad", hip, tangent_wide=True)
    assert aad.wide_route(sc) and float(g["smallest_cir_state"]) - 1e-12 > wa.FLOOR_DISTANCE
    res = sc.run_simulation()
    P = len(g["param_names"])
    assert sc.timings["tangent"] is True and sc.timings["forward_mode_passes"] == (P + NP - 1) // NP and "bumped_passes" not in sc.timings
    assert max(sc.timings["wide_active_slots"]) <= 2, sc.timings["wide_active_slots"]      # a chunk of 4 touches one or two models
    for key in [k for k in g.files if k.startswith("grad_")]:
        ns_i, m_i = (int(x) for x in key.split("_")[1:])
        ref, ours = g[key], np.array(res.derivatives[ns_i][m_i], dtype=np.float64)
        used = ~np.isnan(ref)
        if used.any():
            scale = np.abs(np.where(used, ref, 0.0)).max(axis=1, keepdims=True)
            print(f"WIDE-TANGENT cva10 {key}: worst gap / row's largest entry = "
                  f"{np.max(np.abs(np.where(used, ours - ref, 0.0)) / np.where(scale == 0, 1.0, scale)):.3e}")
    check_lsm_sensitivities(sc, g, res)


def test_cva10_on_three_emulated_ranks_matches_the_single_shard_run(hip):
    import wide_aad_cases as wa
    from emulated_ranks import run_ranks
    from mcx import _native

    def build(be):
        sc, _ = wa.make_controller("wide_cva10_aad", be, inject=False, tangent_wide=True, n_main=6001, n_pre=3002)
        return sc

    single = build(hip)
    ref = _grads(single.run_simulation())
    assert single.timings["tangent"] is True

    def body(sc, rank):
        g = _grads(sc.run_simulation())
        assert sc.timings["tangent"] is True
        return g

    out, calls = run_ranks(3, lambda rank: build(_native.HipBackend(0)), body)
    assert calls["all_reduce"] > 0
    for rank, got in enumerate(out):
        for ns_r, ns_g in zip(ref, got):
            for m_i, (m_r, m_g) in enumerate(zip(ns_r, ns_g)):
                assert np.allclose(m_r, m_g, rtol=1e-9, atol=1e-12), (rank, m_i, np.abs(m_g - m_r).max())


def test_a_hull_white_slot_keeps_the_bump_route_without_a_wasted_base_run(hip, monkeypatch):
    sc = _five_slot_book(hip, True, letters="BHBVCDBVCD", seed=14)
    assert aad._wide_model(sc.model) and not aad.wide_route(sc)
    runs = []
    real = aad.run_with_bumps
    monkeypatch.setattr(aad, "_clone_controller", (lambda f: lambda *a, **k: runs.append(1) or f(*a, **k))(aad._clone_controller))
    sc.run_simulation()
    P = len(sc.model.get_model_params())
    assert real is aad.run_with_bumps and sc.timings["tangent"] is False and sc.timings["bumped_passes"] == 2 * P
    assert len(runs) == 1 + 2 * P, "one base run and 2P bumped runs: the forward-mode pass must not have started a base run"
