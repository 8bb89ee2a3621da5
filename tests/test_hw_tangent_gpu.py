"""Forward-mode sensitivities of Hull-White books on the GPU: the two Hull-White dual steps of the per-slot dual path kernel
(csrc/kt_wide.hip kt_paths_wide<., true> behind mcx_tangent_paths_wide_hw) and the route through it (mcx.aad.hull_white_route,
SimulationController.tangent_hull_white).

Kernel level, with the launch and the assertions of tests/test_wide_tangent_gpu.py on the new entry (value image = generate_paths'
bytes, padding untouched, tangent columns of inactive slots exactly 0, n_active from the tables, the two bounds): a single Hull-White
slot forced wide under EULER and ANALYTICAL, the two-slot mix HC, the 9- and 32-slot mixes of tests/wide_cases.py; 1 / 255 / 257
paths, Philox and injected draws; rate, sigma, mean reversion and the live curve nodes of every Hull-White slot in chunks of 4, and
one chunk of dead nodes (all-zero images, nothing launched).  Bound: 4 x the restatement's own float64-against-long-double gap
(tests/hw_tangent_reference.py), floored at n_sub_steps x 2.2e-16, relative to the row's largest entry, per model, chunk and path count.

Then: two launches split at a path offset, the bytes of mcx_tangent_paths_wide on sims without a Hull-White slot, refusals by code.

End to end: each book with the flag on against the same book on the (now curve-aware) bump route, rows within 4e-6 of the row's
largest entry (the bound of forward against bump in tests/test_wide_tangent_gpu.py); three emulated ranks against one shard."""
import ctypes as C

import numpy as np
import pytest
import torch

import hw_tangent_reference as hw
import test_wide_tangent_gpu as wg
import wide_cases as wc
import wide_tangent_reference as wt
from mcx import _abi, aad

pytestmark = pytest.mark.gpu
NP = _abi.TANGENT_NP
SEED = wg.SEED
NAN = float("nan")
MODELS = {
    "hw_1_euler": (lambda: hw.hw_model(), "EULER"),
    "hw_1_analytical": (lambda: hw.hw_model(), "ANALYTICAL"),
    "hc_2_euler": (lambda: wc.mixed_model("HC", 4), "EULER"),
    "mix_9_euler": wc.WIDE["mix_9_euler"],
    "mix_32_euler": wc.WIDE["mix_32_euler"],
}
_CACHE = {}


class _HwEntry:
    """the backend with `tangent_paths_wide` served by mcx_tangent_paths_wide_hw: the helpers of tests/test_wide_tangent_gpu.py then
    launch, and check, the new entry"""

    def __init__(self, hip):
        self._hip = hip

    def __getattr__(self, name):
        return getattr(self._hip, name)

    def tangent_paths_wide(self, *a, **k):
        return self._hip.tangent_paths_wide_hw(*a, **k)


def _setup(hip, name):
    from mcx.common.enums import SimulationScheme
    from mcx.plan import SimPlan
    if name not in _CACHE:
        build, scheme = MODELS[name]
        model = build()
        plan = SimPlan(model, wc.TIMELINE, SimulationScheme[scheme], wc.NUM_STEPS, force_wide=True)
        _CACHE[name] = (model, plan, plan.create_sim(hip), hw.derivative_tables(model, plan))
    return _CACHE[name]


def _hull_white_chunks(model, plan, dd):
    """[(parameter indices, padded tables)] — per Hull-White leaf its live parameters in chunks of NP — and one chunk of dead ones"""
    live = hw.expected_live(model, np.asarray(plan.steps["t1"], dtype=np.float64))
    assert live == [j for j in aad.live_parameters(dd) if j in live], "a parameter the geometry calls live has no tangent anywhere"
    sels = []
    for off, leaf in hw.hull_white_leaves(model):
        own = [j for j in live if off <= j < off + len(leaf.model_params)]
        assert own == [j for j in aad.live_parameters(dd) if off <= j < off + len(leaf.model_params)], "the geometry's list is the tables'"
        assert own[:3] == [off, off + 1, off + 2] and len(own) > 3
        sels += [own[c0:c0 + NP] for c0 in range(0, len(own), NP)]
    off, leaf = hw.hull_white_leaves(model)[0]
    dead = [j for j in range(off, off + len(leaf.model_params)) if j not in live][:NP]
    assert len(dead) == NP and not any(np.any(v[..., dead] != 0) for v in dd.values())
    pad = lambda sel: dict({k: aad.pad_chunk(v, sel) for k, v in dd.items()}, **({} if "chol" in dd else {"chol": None}))
    return [(sel, pad(sel)) for sel in sels], (dead, pad(dead))


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inject", [False, True], ids=["philox", "injected"])
@pytest.mark.parametrize("name", list(MODELS))
def test_kernel_against_the_restatement_with_explicit_tangents(name, inject, hip):
    model, plan, sim, dd = _setup(hip, name)
    be = _HwEntry(hip)
    assert plan.wide and hip.sim_describe(sim)["signature"] == "WIDE" and ("chol" in dd) == name.endswith("analytical")
    n_max = max(wc.N_PATHS)
    z = np.random.default_rng(17).standard_normal((plan.n_steps, plan.n_z, n_max)) if inject else wg._device_normals(hip, plan, n_max)
    chunks, (dead, d_dead) = _hull_white_chunks(model, plan, dd)
    hw_slots = [r for r, sl in enumerate(wt.wr.slot_records(plan)) if sl["kind"] == hw.HW]
    worst_own = worst_gap = worst_gap_n = 0.0
    acts = []
    for sel, d in chunks:
        own, hi = hw.own_rounding(plan, z, d["slots"], d["init"], d["aux"], d["chol"])
        assert hi.min_floor_gap > 1e-9, (name, sel, "a CIR++ path comes near its floor or 0", hi.min_floor_gap)
        assert np.abs(hi.dpaths[:len(sel)]).reshape(len(sel), -1).max(axis=1).min() > 0, (name, sel, "a live parameter without a tangent")
        for n in wc.N_PATHS:
            gap, gap_n, n_active = wg._check_chunk(be, name, plan, sim, sel, d, n, z, hi, own, inject)
            assert n_active == 1
            worst_gap, worst_gap_n = max(worst_gap, gap), max(worst_gap_n, gap_n)
        worst_own = max(worst_own, own)
        acts += wt.active_from_tables(plan, d["slots"], d["init"], d["aux"], d["chol"])
    print(f"HW-TANGENT {name} {'injected' if inject else 'philox'}: {len(chunks)} chunks, largest yardstick {worst_own:.3e}, "
          f"worst device gap {worst_gap:.3e} (on the scale of the launch's own paths {worst_gap_n:.3e}); active slots {acts}")
    assert sorted(set(acts)) == hw_slots, "every Hull-White slot, and only those"
    for n in wc.N_PATHS:                                   # dead curve nodes: nothing is active, every image is zero
        paths, dpaths, n_active = wg._launch(be, sim, d_dead, n)
        assert n_active == 0 and not dpaths.cpu().numpy().any(), (name, dead)
        assert torch.equal(paths, hip.generate_paths(sim, SEED, 0, n))


@pytest.mark.parametrize("off", [5, 2 ** 33 + 5])
@pytest.mark.parametrize("name", ["hc_2_euler", "hw_1_analytical"])
def test_two_launches_split_at_a_path_offset_give_the_bytes_of_one(name, off, hip):
    model, plan, sim, dd = _setup(hip, name)
    n, cut = 257, 100
    sel, d = _hull_white_chunks(model, plan, dd)[0][0]
    call = lambda o, m, out, z=None: hip.tangent_paths_wide_hw(sim, d["slots"], d["init"], d["aux"], d["chol"], SEED, o, m, z, out=out,
                                                               ld=n + wc.LD_PAD)
    z = torch.zeros((plan.n_steps, plan.n_z, n + wc.LD_PAD), dtype=torch.float64, device=hip.device)
    z[:, :, :n] = hip.from_numpy(np.random.default_rng(9).standard_normal((plan.n_steps, plan.n_z, n)))
    for inject in (False, True):
        (bp, bd), whole = wg._padded(hip, plan, n)
        call(off, n, whole, z if inject else None)
        (sp, sd), _v = wg._padded(hip, plan, n)
        call(off, cut, (sp[:, :, :cut], sd[:, :, :, :cut]), z if inject else None)
        call(off + cut, n - cut, (sp[:, :, cut:n], sd[:, :, :, cut:n]), z[:, :, cut:] if inject else None)
        hip.synchronize()
        assert torch.equal(sp[:, :, :n], bp[:, :, :n]) and torch.equal(sd[:, :, :, :n], bd[:, :, :, :n]), (name, off, inject)
        assert bd[:, :, :, :n].abs().max() > 0
        assert torch.isnan(sp[:, :, n:]).all() and torch.isnan(sd[:, :, :, n:]).all()


@pytest.mark.parametrize("name", ["vbcd_9_euler", "bs_12_analytical"])
def test_a_sim_without_a_hull_white_slot_gets_the_bytes_of_the_plain_entry(name, hip):
    model, plan, sim, dd = wg._setup(hip, name)
    n = 257
    for sel, d in list(wt.chunks(dd, len(model.get_model_params()), NP))[:3]:
        args = (sim, d["slots"], d["init"], d["aux"], d["chol"], SEED, 3, n)
        p0, d0, a0 = hip.tangent_paths_wide(*args)
        p1, d1, a1 = hip.tangent_paths_wide_hw(*args)
        assert a0 == a1 > 0 and torch.equal(p0, p1) and torch.equal(d0, d1) and d0.abs().max() > 0, (name, sel)


def _raw_call(hip, sim, plan, n, ld=None, dchol="zeros", paths=None, dpaths=None):
    dslot, dinit = np.zeros((plan.n_slots, _abi.SLOT_NPARAM, NP)), np.zeros((plan.n_state, NP))
    daux = np.zeros((plan.n_steps, plan.n_slots, _abi.AUX, NP))
    dslot[0, 1, 0] = 1.0                                    # an active slot: an accepted call would launch
    dc = np.zeros((max(len(plan.chol), 1), plan.n_z, plan.n_z, NP)) if dchol == "zeros" else None
    return hip.lib.mcx_tangent_paths_wide_hw(hip.h, sim.ptr, _abi.ptr(dslot), _abi.ptr(dinit), _abi.ptr(daux), _abi.ptr(dc) if dc is not None else None,
                                             SEED, 0, n, paths.data_ptr(), dpaths.data_ptr(), n if ld is None else ld, None, None, None)


def test_refusals_write_nothing(hip):
    from mcx.common.enums import SimulationScheme
    from mcx.plan import SimPlan
    n = 64
    E, A, Q = SimulationScheme.EULER, SimulationScheme.ANALYTICAL, SimulationScheme.QE

    def poisoned(plan):
        return (torch.full((plan.n_dates, plan.n_state, n), NAN, dtype=torch.float64, device=hip.device),
                torch.full((NP, plan.n_dates, plan.n_state, n), NAN, dtype=torch.float64, device=hip.device))

    def call(plan, scheme=None, **kw):
        sim = plan.create_sim(hip)
        if scheme is not None:                     # a scheme no plan of the model has: the descriptor edited, as the library sees it
            desc, out = _abi.WideSimDesc.from_buffer_copy(plan.desc), C.c_void_p()
            desc.scheme = scheme
            assert hip.lib.mcx_sim_create_wide(hip.h, C.byref(desc), C.byref(out)) == 0
            sim = type(sim)(out, hip.lib.mcx_sim_destroy, plan)
        p, d = poisoned(plan)
        rc = _raw_call(hip, sim, plan, n, paths=p, dpaths=d, **kw)
        hip.synchronize()
        return rc, p, d

    def refused(plan, code, word=None, **kw):
        rc, p, d = call(plan, **kw)
        assert rc == code, (rc, code, hip.lib.mcx_last_error(hip.h))
        assert torch.isnan(p).all() and torch.isnan(d).all(), "a refused call wrote"
        if word:
            assert word in hip.lib.mcx_last_error(hip.h).decode(), hip.lib.mcx_last_error(hip.h)

    who = "mcx_tangent_paths_wide_hw"
    refused(SimPlan(hw.hw_model(), wc.TIMELINE, E, wc.NUM_STEPS), _abi.E_NOT_FUSABLE, "narrow")            # a narrow sim
    refused(SimPlan(wc.mixed_model("D" * 9, 5), wc.TIMELINE, E, wc.NUM_STEPS), _abi.E_NOT_FUSABLE, "scheme", scheme=Q.value)   # QE
    hw_a = SimPlan(hw.hw_model(), wc.TIMELINE, A, wc.NUM_STEPS, force_wide=True)
    refused(hw_a, -1, dchol=None)                                                                          # ANALYTICAL without h_dchol
    refused(hw_a, -2, "ld < n_paths", ld=n - 1)
    refused(wc.plan_of("mix_9_euler"), -2, who, ld=n - 1)                                                  # (the message names the entry)
    # ANALYTICAL next to a kind without an analytic step: still refused
    refused(SimPlan(wc.mixed_model("H" + "D" * 8, 5), wc.TIMELINE, E, wc.NUM_STEPS), _abi.E_NOT_FUSABLE, "analytic tangent step", scheme=A.value)
    for plan in (hw_a, wc.plan_of("mix_9_euler")):                                                         # and what it accepts
        rc, p, d = call(plan)
        assert rc == 0 and not torch.isnan(p).any() and not torch.isnan(d).any()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _rows(res):
    return [np.array(m, dtype=np.float64) for m in res.derivatives[0]]


def _forward_against_bump(tag, fwd, bump, hw_params):
    """run the book with the flag on and off; -> (forward controller, bumped controller).  hw_params: (first index, leaf) of the
    Hull-White leaf the book reads"""
    fwd.tangent_hull_white = True
    assert aad.hull_white_route(fwd) and not aad.hull_white_route(bump) and bump.tangent_hull_white is False
    g_f, g_b = _rows(fwd.run_simulation()), _rows(bump.run_simulation())
    P = len(fwd.model.get_model_params())
    dead = fwd.timings["dead_parameters"]
    assert fwd.timings["tangent"] is True and "bumped_passes" not in fwd.timings and fwd.sim_plan.wide
    assert fwd.timings["forward_mode_passes"] == (P - len(dead) + NP - 1) // NP == len(fwd.timings["wide_active_slots"])
    assert bump.timings["tangent"] is False and bump.timings["bumped_passes"] == 2 * P
    off, leaf = hw_params
    n = len(leaf._t)
    live = hw.expected_live(leaf, np.asarray(fwd.sim_plan.steps["t1"], dtype=np.float64), atoms_to=1.0)
    assert [j - off for j in dead if off <= j < off + 3 + 2 * n] == [j for j in range(3 + 2 * n) if j not in live], dead
    for m_i, (a, b) in enumerate(zip(g_f, g_b)):
        scale = np.abs(b).max(axis=1, keepdims=True)
        gap = np.abs(a - b) / np.where(scale == 0, 1.0, scale)
        print(f"HW-TANGENT {tag}, metric {m_i}: forward against bumped over {fwd.timings['forward_mode_passes']} passes "
              f"({len(dead)} of {P} parameters dead), worst gap / row's largest entry = {gap.max():.3e}")
        assert np.all(gap <= 4e-6), (tag, m_i, gap.max())
        assert not a[:, dead].any() and not b[:, dead].any(), "a dead parameter has exact-zero rows on both routes"
    curve = [off + j for j in live if j >= 3]
    assert all(np.any(g_b[0][:, j] != 0) and np.any(g_f[0][:, j] != 0) for j in curve), "the live curve-node rows are non-zero"
    return fwd, bump


@pytest.mark.parametrize("scheme", ["EULER", "ANALYTICAL"])
def test_bermudan_swaption_under_a_single_hull_white_model(scheme, hip):
    fwd, bump = hw.exercise_book(hip, scheme), hw.exercise_book(hip, scheme)
    fwd, _ = _forward_against_bump(f"bermudan {scheme}", fwd, bump, (0, fwd.model))
    assert fwd.timings["forward_mode_passes"] == 3 and fwd.timings["dead_parameters"] == [6, 7, 8, 12, 13, 14]
    assert fwd.timings["wide_active_slots"] == [1, 1, 1]


def test_swap_netting_set_under_hull_white_and_cirpp(hip):
    fwd, bump = hw.cva_book(hip), hw.cva_book(hip)
    fwd, _ = _forward_against_bump("swap + bond CVA", fwd, bump, (0, fwd.model.models[0]))
    assert fwd.timings["forward_mode_passes"] == 4 and max(fwd.timings["wide_active_slots"]) <= 2      # 9 + 4 live parameters


def _ten_slot_book(hip):
    """the book of wg._five_slot_book on the ten slots BHBVCDBVCD, with the payer swap on the Hull-White short rate (slot 1)"""
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    mod = wc.mcx_classes()
    model = wc.mixed_model("BHBVCDBVCD", 14, mod)
    assert model.models[1].asset_ids == ["hw1"]
    call = mod["EuropeanOption"](mod["Equity"]("eq0"), 1.0, 85.0, mod["OptionType"].CALL, asset_id="eq0")
    call.name = "call"
    swap = mod["InterestRateSwap"](0.0, 1.0, 1.0, 0.03, 0.5, 0.5, mod["IRSType"].PAYER, "hw1")
    swap.name = "swap"
    ns = [mod["NettingSet"](name="book", products=[call, swap])]
    rm = mod["RiskMetrics"]([mod["PVMetric"](), mod["EPEMetric"]()], exposure_timeline=np.array([0.0, 0.5, 1.0]))
    return SimulationController(ns, model, rm, 4096, 2048, 2, SimulationScheme.EULER, differentiate=True, backend=hip)


def test_ten_slot_book_with_a_hull_white_slot(hip):
    fwd, bump = _ten_slot_book(hip), _ten_slot_book(hip)
    assert aad._wide_model(fwd.model)
    fwd, _ = _forward_against_bump("ten slots", fwd, bump, (3, fwd.model.models[1]))
    P = len(fwd.model.get_model_params())
    assert P == 88 and len(fwd.timings["dead_parameters"]) >= 48                                        # 24 + 24 curve nodes beyond the year


def test_cva_book_on_three_emulated_ranks_matches_the_single_shard_run(hip):
    from emulated_ranks import run_ranks
    from mcx import _native

    def build(be):
        sc = hw.cva_book(be, n_main=601, n_pre=302)
        sc.tangent_hull_white = True
        return sc

    single = build(hip)
    ref = wg._grads(single.run_simulation())
    assert single.timings["tangent"] is True

    def body(sc, rank):
        g = wg._grads(sc.run_simulation())
        assert sc.timings["tangent"] is True and sc.timings["forward_mode_passes"] == 4
        return g

    out, calls = run_ranks(3, lambda rank: build(_native.HipBackend(0)), body)
    assert calls["all_reduce"] > 0
    for rank, got in enumerate(out):
        for ns_r, ns_g in zip(ref, got):
            for m_i, (m_r, m_g) in enumerate(zip(ns_r, ns_g)):
                assert np.allclose(m_r, m_g, rtol=1e-9, atol=1e-12), (rank, m_i, np.abs(m_g - m_r).max())
