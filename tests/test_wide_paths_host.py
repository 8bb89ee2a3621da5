"""Wide models, host side (no GPU): the descriptor SimPlan builds for more than MCX_MAX_SLOTS sub-models, the unchanged narrow
descriptors, the backends without a wide kernel, the gates that send a wide book's sensitivities to bump-and-revalue."""
import ctypes as C

import numpy as np
import pytest

import cases
import wide_cases as wc
from mcx import _abi, aad
from mcx.common.enums import SimulationScheme
from mcx.plan import SimPlan

TL = np.array([0.0, 0.5, 1.25])
COUNTS = ("scheme", "n_slots", "n_state", "n_z", "n_uniform", "n_steps", "n_dates", "n_chol", "n_initial_store", "flags")


def _arr_ptr(a):
    return a.ctypes.data if a.size else _abi.ptr(a).value


@pytest.mark.parametrize("name", ["mix_9_euler", "mix_32_euler", "bs_12_analytical", "bs_32_analytical"])
def test_wide_descriptor_round_trips(name):
    plan = wc.plan_of(name)
    build, scheme = wc.WIDE[name]
    specs = build()._slots()
    d = plan.desc
    assert plan.wide and isinstance(d, _abi.WideSimDesc) and len(specs) == plan.n_slots > _abi.MAX_SLOTS
    assert (d.scheme, d.n_slots, d.n_z, d.n_uniform) == (SimulationScheme[scheme].value, len(specs), len(specs), 0)
    assert d.n_state == sum(s.state_dim for s in specs) == plan.n_state <= _abi.WIDE_MAX_STATE
    assert (d.n_steps, d.n_dates, d.n_initial_store) == (4, 3, 1)
    assert d.n_chol == len(plan.chol) == (2 if scheme == "ANALYTICAL" else 1) and plan.chol.shape[1:] == (plan.n_z, plan.n_z)
    assert plan.aux.shape == (4, plan.n_slots, _abi.AUX)
    # the pointers are those of the arrays the plan keeps alive
    assert d.slots == C.addressof(plan.slot_records) and C.sizeof(plan.slot_records) == plan.n_slots * C.sizeof(_abi.Slot)
    assert (d.steps, d.chol, d.aux, d.init_state) == (plan.steps.ctypes.data, plan.chol.ctypes.data, plan.aux.ctypes.data,
                                                        plan.init_state.ctypes.data)
    # the records read back through the pointer, as the library reads them
    recs = C.cast(d.slots, C.POINTER(_abi.Slot))
    so = 0
    for i, s in enumerate(specs):
        assert (recs[i].kind, recs[i].state_off, recs[i].z_off, recs[i].flags) == (s.kind, so, i, s.flags)
        assert [recs[i].p[j] for j in range(_abi.SLOT_NPARAM)] == list(s.params) + [0.0] * (_abi.SLOT_NPARAM - len(s.params))
        assert s.sim_dim == 1 and s.kind in _abi.WIDE_KINDS
        so += s.state_dim
    assert np.array_equal(plan.init_state, np.array(build()._initial_state()))
    for k in range(plan.n_steps):
        L = plan.chol[plan.steps["chol_idx"][k]]
        assert np.array_equal(L, np.tril(L)) and (np.diag(L) > 0).all()
        if scheme == "EULER":
            assert L[0, 0] == 1.0 and plan.steps["chol_idx"][k] == 0
    assert len(set(plan.steps["dt"])) == 2


def test_limits_of_a_wide_plan():
    assert (_abi.WIDE_MAX_SLOTS, _abi.WIDE_MAX_STATE, _abi.MAX_SLOTS, _abi.MAX_Z, _abi.MAX_STATE) == (32, 64, 8, 8, 16)
    assert _abi.SIG_NAMES[9] == "WIDE"
    E = SimulationScheme.EULER
    assert SimPlan(wc.bs_multi(32, 1), TL, E, 1).wide
    with pytest.raises(ValueError, match="MCX_WIDE_MAX_SLOTS"):
        SimPlan(wc.bs_multi(33, 1), TL, E, 1)
    # exactly MCX_MAX_SLOTS sub-models stay on the narrow route unless forced
    assert not SimPlan(wc.bs_multi(8, 1), TL, E, 1).wide and SimPlan(wc.bs_multi(8, 1), TL, E, 1, force_wide=True).wide
    # a sub-model with two factors has no place in a wide model
    _ns, heston, _rm = cases.heston()
    with pytest.raises(ValueError, match="MCX_WIDE_MAX_SLOTS"):
        SimPlan(heston, TL, E, 1, force_wide=True)
    _ns, s2f, _rm = cases.s2f_european()
    with pytest.raises(ValueError, match="MCX_WIDE_MAX_SLOTS"):
        SimPlan(s2f, TL, E, 1, force_wide=True)
    # the single-step plan of Model.simulate_time_step_* follows the model's width
    _ns, model, _rm = wc.cva10(wc.mcx_classes())
    one = SimPlan.single_step(model, E, 0.3, 0.55)
    assert one.wide and one.n_steps == 1 and np.array_equal(one.chol[0], np.eye(10))


def test_struct_sizes():
    assert C.sizeof(_abi.Slot) == 80
    assert C.sizeof(_abi.SimDesc) == 10 * 4 + _abi.MAX_SLOTS * 80 + 4 * 8 == 712          # unchanged: MCX_ABI_VERSION stays 6
    assert C.sizeof(_abi.WideSimDesc) == 10 * 4 + 5 * 8 == 80
    assert _abi.ABI_VERSION == 6
    assert [f[0] for f in _abi.WideSimDesc._fields_] == [f[0] for f in _abi.SimDesc._fields_]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_narrow_plans_are_byte_for_byte_what_they_were(name):
    """every case of tests/cases.py: plan.wide is False and the SimDesc holds, field by field and byte by byte, what the
    constructor computes for a model of 1 .. 8 slots — the fill of the descriptor before wide models existed, restated here"""
    build, _n_pre, _n_main, steps, scheme, _diff = cases.CASES[name]
    _ns, model, _rm = build()
    plan = SimPlan(model, TL, scheme, steps)
    d = plan.desc
    assert plan.wide is False and type(d) is _abi.SimDesc and not hasattr(plan, "slot_records")
    specs = model._slots()
    n_state, n_z = sum(s.state_dim for s in specs), sum(s.sim_dim for s in specs)
    want = _abi.SimDesc()
    want.scheme, want.n_slots, want.n_state, want.n_z = scheme.value, len(specs), n_state, n_z
    want.n_uniform, want.n_steps, want.n_dates, want.n_chol = plan.n_uniform, 2 * steps, 3, len(plan.chol)
    want.n_initial_store, want.flags = 1, _abi.FLAG_SMOOTHING if model.perform_smoothing else 0
    so = zo = 0
    for i, s in enumerate(specs):
        want.slots[i].kind, want.slots[i].state_off, want.slots[i].z_off, want.slots[i].flags = s.kind, so, zo, s.flags
        for j, v in enumerate(s.params):
            want.slots[i].p[j] = v
        so += s.state_dim
        zo += s.sim_dim
    want.steps, want.chol, want.aux, want.init_state = (_arr_ptr(plan.steps), _arr_ptr(plan.chol), _arr_ptr(plan.aux),
                                                        _arr_ptr(plan.init_state))
    for f in COUNTS + ("steps", "chol", "aux", "init_state"):
        assert getattr(d, f) == getattr(want, f), (name, f)
    for i in range(_abi.MAX_SLOTS):
        assert bytes(d.slots[i]) == bytes(want.slots[i]), (name, "slot", i)
    assert bytes(d) == bytes(want) and len(bytes(d)) == 712
    assert (plan.n_slots, plan.n_state, plan.n_z, plan.n_steps) == (len(specs), n_state, n_z, 2 * steps)


def test_a_backend_without_the_wide_kernel_refuses_the_plan(oracle):
    from mcx.engine.engine import MonteCarloEngine
    assert not getattr(oracle, "supports_wide", False)
    plan = wc.plan_of("mix_9_euler")
    with pytest.raises(ValueError, match="mcx_sim_create_wide"):
        plan.create_sim(oracle)
    with pytest.raises(ValueError, match="mcx_sim_create_wide"):
        wc.plan_of("vas_cir_2_euler", force_wide=True).create_sim(oracle)
    assert wc.plan_of("vas_cir_2_euler").create_sim(oracle).plan.wide is False          # narrow plans run as before
    with pytest.raises(ValueError, match="mcx_sim_create_wide"):
        MonteCarloEngine(wc.TIMELINE, SimulationScheme.EULER, wc.mixed_model("VBCHDVBCHD", 3), 16, 1, backend=oracle)
    sc, _ = wc.make_controller("wide_cva10", oracle, inject=False)
    with pytest.raises(ValueError, match="mcx_sim_create_wide"):
        sc.run_simulation()


def test_sensitivities_of_a_wide_book_go_to_bumps(oracle, monkeypatch):
    """the host gates: no tangent kernel and no forward-mode route is tried for a wide model, run_simulation(differentiate=True)
    goes straight to bump-and-revalue"""
    sc, _ = wc.make_controller("wide_basket12_analytical_aad", oracle, inject=False)
    assert sc.differentiate and aad._wide_model(sc.model) and not aad._wide_model(cases.basket_multi()[1])
    assert not aad.tangent_kernels_apply(sc)
    with pytest.raises(NotImplementedError, match="wide model"):
        aad._check_supported(sc)
    with pytest.raises(aad._NoTangentForm, match="wide model"):
        aad._tangent_book_routes(sc)
    narrow, _ = cases.make_controller("mixed_cva_aad", oracle)
    aad._tangent_book_routes(narrow)                                                    # (a narrow book passes the same gate)
    called = []
    monkeypatch.setattr(aad, "run_with_bumps", lambda c: called.append("bumps") or "bumped")
    monkeypatch.setattr(aad, "run_with_tangent_book", lambda c: aad._tangent_book_routes(c) and called.append("tangent book"))
    monkeypatch.setattr(aad, "run_with_tangents", lambda c: called.append("tangents"))
    oracle.tangent_paths = None                     # a backend that has the forward-mode entry points: the gate is the host's
    try:
        assert sc.run_simulation() == "bumped" and called == ["bumps"]
    finally:
        del oracle.tangent_paths
