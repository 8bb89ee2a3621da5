"""Host side of the gas storage (mcx/products/storage.py, storage_helpers.py; no GPU): window optimiser, transitions, timeline,
the compat import path, the loud errors, and the byte layout of the new ABI structs.  Fixture values are the reference's
(tests/golden/gen_storage_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import storage_cases
from mcx import _abi
from mcx.products.storage import ACTION_ORDER, Storage, StorageAction
from mcx.products.storage_helpers import StorageConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _storages(name):
    ns, model, rm = storage_cases.CASES[name][0](storage_cases.mcx_classes())
    prods = [p for n in ns for p in n.products]
    return [(i, p) for i, p in enumerate(prods) if isinstance(p, Storage)]


@pytest.mark.parametrize("name", list(storage_cases.CASES))
def test_optimised_windows_equal_the_reference_exactly(name):
    g = storage_cases.load_golden(name)
    for i, p in _storages(name):
        ours = np.array([[w.vmin, w.vmax] for w in p.storage_config.volume_constraints])
        assert np.array_equal(ours, g[f"windows_{i}"]), (name, i)


def test_shifting_windows_run_the_bisection():
    """[0,12] -> [2,10] -> [0,6]: boundaries moved backwards (not one of the configured values), first window pinned"""
    (_, p), = _storages("storage_shift")
    w = p.storage_config.volume_constraints
    assert (w[0].vmin, w[0].vmax) == (4.0, 4.0)
    assert any(x.vmax not in (12.0, 10.0, 6.0) and x.vmax < 12.0 for x in w[1:])
    assert len(w) == len(p.product_timeline) + 1


def test_unsatisfiable_windows_raise():
    c = StorageConfig()
    c.add_volume_constraint(0.0, 1.0, 0.0, 12.0, 0.0)
    c.add_volume_constraint(1.0, 3.0, 10.0, 12.0, 0.0)          # 10 units by day 1 at 1 unit a day from 4
    c.add_injection_flexibility(0.0, 3.0, 0.0, 1.0)
    c.add_withdrawal_flexibility(0.0, 3.0, 0.0, 1.0)
    c.add_variable_injection_cost(0.0, 0.0)
    c.add_variable_withdrawal_cost(0.0, 0.0)
    with pytest.raises(ValueError, match="Initial volume constraints cannot be satisfied at date"):
        Storage("gas", 0.0, 3.0, 4.0, c, 4)
    with pytest.raises(ValueError, match="at least two discrete states"):
        Storage("gas", 0.0, 3.0, 4.0, StorageConfig(), 1)
    with pytest.raises(ValueError, match="Rollout interval must be positive"):
        Storage("gas", 0.0, 3.0, 4.0, StorageConfig(), 4, 0.0)


@pytest.mark.parametrize("name", list(storage_cases.CASES))
def test_transition_tables_match_the_reference(name):
    g = storage_cases.load_golden(name)
    for i, p in _storages(name):
        ref = g[f"trans_{i}"]
        ours = p._transition_table()
        assert ours.shape == ref.shape
        assert np.abs(ours - ref).max() <= 1e-12
        # the public maps, action by action, and state -> volume -> state
        states = torch.arange(p.num_states, dtype=torch.float64)
        for j, (t, nxt) in enumerate(zip(p.product_timeline.tolist(), p.next_action_dates.tolist())):
            for a, act in enumerate(ACTION_ORDER):
                ns = p.compute_next_state(t, nxt, act)(states)
                dv = p.compute_volume_difference(t, nxt, act)(states)
                assert np.abs(ns.numpy() - ref[j, :, a, 0]).max() <= 1e-12 and np.abs(dv.numpy() - ref[j, :, a, 1]).max() <= 1e-12
                assert torch.allclose(p.state_to_volume(nxt, ns) - p.state_to_volume(t, states), dv, atol=1e-10, rtol=0.0)
        d = p._device_dates()
        assert d["is_last"].tolist() == [0] * (len(d) - 1) + [1]
        assert np.array_equal(d["vmin"], g[f"windows_{i}"][:-1, 0]) and np.array_equal(d["next_vmax"], g[f"windows_{i}"][1:, 1])


# ---- the host-only properties of the reference's test_storage.py:64-113, restated ----------------------------------------
def _constant_window_storage():
    c = StorageConfig()
    c.add_volume_constraint(0.0, 4.0, 0.0, 12.0, 0.0)
    c.add_injection_flexibility(0.0, 4.0, 0.0, 3.0)
    c.add_injection_flexibility(0.0, 4.0, 6.0, 1.5)
    c.add_withdrawal_flexibility(0.0, 4.0, 0.0, 1.0)
    c.add_withdrawal_flexibility(0.0, 4.0, 6.0, 2.5)
    c.add_variable_injection_cost(0.0, 1.0)
    c.add_variable_withdrawal_cost(0.0, 1.0)
    return Storage("thegasprice", 0.0, 4.0, 4.0, c, 4)


def test_injection_is_monotone_and_capacity_limited():
    p = _constant_window_storage()
    s = torch.tensor([0.0, 1.0, 2.0, 3.0], dtype=torch.float64)
    ns = p.compute_next_state(1.0, 2.0, StorageAction.INJECTION)(s)
    nv = p.state_to_volume(2.0, ns)
    assert torch.all(ns[1:] >= ns[:-1]) and torch.all(nv >= p.state_to_volume(1.0, s))
    assert torch.allclose(nv, torch.tensor([4.5, 5.5, 6.5, 7.5], dtype=torch.float64), atol=1e-10, rtol=0.0)
    assert nv[-1].item() == p.storage_config.get_volume_constraint(2.0).vmax


def test_hold_projects_the_inventory_into_the_next_window():
    c = StorageConfig()
    for w in ((0.0, 2.0, 0.0, 12.0), (2.0, 3.0, 0.0, 12.0), (3.0, 4.0, 3.0, 9.0)):
        c.add_volume_constraint(*w, 0.0)
    c.add_injection_flexibility(0.0, 4.0, 0.0, 3.0)
    c.add_withdrawal_flexibility(0.0, 4.0, 0.0, 3.0)
    c.add_variable_injection_cost(0.0, 0.0)
    c.add_variable_withdrawal_cost(0.0, 0.0)
    p = Storage("thegasprice", 0.0, 4.0, 6.0, c, 4)
    s = torch.tensor([0.0, 1.0, 2.0, 3.0], dtype=torch.float64)
    held = p.compute_next_state(2.0, 3.0, StorageAction.DO_NOTHING)(s)
    assert torch.allclose(p.state_to_volume(3.0, held), torch.tensor([3.0, 4.0, 8.0, 9.0], dtype=torch.float64), atol=1e-10, rtol=0.0)
    assert held[1].item() == 0.5 and held[2].item() == 2.5


def test_volume_difference_is_the_physical_change():
    p = _constant_window_storage()
    s = torch.tensor([0.0, 1.0, 2.0, 3.0], dtype=torch.float64)
    for act in StorageAction:
        ns = p.compute_next_state(1.0, 2.0, act)(s)
        assert torch.allclose(p.compute_volume_difference(1.0, 2.0, act)(s), p.state_to_volume(2.0, ns) - p.state_to_volume(1.0, s),
                              atol=1e-10, rtol=0.0)


def test_lookups_fall_back_to_the_last_entry_and_costs_step_from_the_left():
    (_, p), = _storages("storage_const")
    c = p.storage_config
    assert c.get_initial_volume_constraint(99.0) is c.initial_volume_constraints[-1]
    assert c.get_injection_flexibility_slice(99.0) is c.injection_flexibility[-1].values
    assert [c.get_variable_injection_cost(t) for t in (-1.0, 0.0, 3.9, 4.0, 7.0)] == [0.2, 0.2, 0.2, 0.3, 0.3]
    assert c.get_injection_flexibility_rate(0.0, 3.0) == 2.25 and c.get_injection_flexibility_rate(0.0, 11.0) == 0.5
    v = torch.tensor([-1.0, 3.0, 6.0, 8.0, 11.0], dtype=torch.float64)
    assert c.interpolate_rate_tensor(v, c.get_injection_flexibility_slice(0.0)).tolist() == [3.0, 2.25, 1.5, 1.0, 0.5]


def test_timeline_and_request_layout():
    (_, p), = _storages("storage_short_last")
    assert p.product_timeline.tolist() == [0.0, 2.0, 4.0, 6.0] and p.next_action_dates.tolist() == [2.0, 4.0, 6.0, 7.5]
    assert p.modeling_timeline is p.product_timeline and p.regression_timeline is p.product_timeline
    assert sorted(p.numeraire_requests) == [0, 1, 2, 3] and sorted(p.spot_requests) == [(j, "gas") for j in range(4)]
    assert [r.time1 for r in p.numeraire_requests.values()] == [0.0, 2.0, 4.0, 6.0]
    assert p.get_num_states() == 6 and p.get_initial_state() == 0.0 and p.get_state_dtype() == torch.float64
    assert p._cash_events(None) == []


def test_compat_import_path():
    import importlib
    import sys
    import mcx.compat
    saved = dict(sys.modules)
    try:
        mcx.compat.install()
        mod = importlib.import_module("products.storage")
        assert mod.Storage is Storage and importlib.import_module("products.storage_helpers").StorageConfig is StorageConfig
    finally:
        for k in list(sys.modules):
            if k not in saved:
                del sys.modules[k]


def test_backends_without_the_entry_points_and_differentiation_fail_loudly():
    from oracle_backend import OracleBackend
    sc, _ = storage_cases.make_controller("storage_const", OracleBackend(), inject=False)
    with pytest.raises(NotImplementedError, match="HIP backend"):
        sc.run_simulation()
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    ns, model, rm = storage_cases.storage_const(storage_cases.mcx_classes())
    with pytest.raises(NotImplementedError, match="storage policy"):
        SimulationController(ns, model, rm, 64, 64, 1, SimulationScheme.ANALYTICAL, True, backend=OracleBackend())


def test_too_many_states_or_knots_are_refused_on_the_host():
    from oracle_backend import OracleBackend
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    mod = storage_cases.mcx_classes()
    p = storage_cases._daily_store(mod, _abi.STORAGE_MAX_STATES + 1, 8.0, [(0.0, 9.0, 0.0, 12.0)])
    with pytest.raises(ValueError, match="MCX_STORAGE_MAX_STATES"):
        SimulationController([mod["NettingSet"](name="st", products=[p])], storage_cases._gas_model(mod), mod["RiskMetrics"]([mod["PVMetric"]()]),
                             64, 64, 1, SimulationScheme.ANALYTICAL, False, backend=OracleBackend())
    q = storage_cases._daily_store(mod, 4, 8.0, [(0.0, 9.0, 0.0, 12.0)])
    for k in range(_abi.STORAGE_MAX_KNOTS):
        q.storage_config.add_injection_flexibility(0.0, 9.0, 10.5 + 0.1 * k, 0.4)
    with pytest.raises(ValueError, match="MCX_STORAGE_MAX_KNOTS"):
        q._device_dates()


def test_new_struct_layouts_match_the_header():
    """sizes from the header's field lists (8-byte doubles / int64 / pointers, 4-byte int32), against the ctypes / numpy mirrors"""
    text = open(os.path.join(ROOT, "include", "mcx.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (MCX_STORAGE_MAX_\w+)\s+(\d+)", text)}
    assert consts == {"MCX_STORAGE_MAX_STATES": _abi.STORAGE_MAX_STATES, "MCX_STORAGE_MAX_KNOTS": _abi.STORAGE_MAX_KNOTS}
    assert _abi.STORAGE_MAX_STATES >= 32 and _abi.MAX_STATES == 8

    def size_of(name):
        body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        total = 0
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            width = 4 if decl.startswith("int32_t") else 8
            for item in decl.split(",") if "*" not in decl else [decl]:
                dims = re.findall(r"\[(\w+)\]", item)
                total += width * int(np.prod([consts.get(d_) or int(d_) for d_ in dims])) if dims else width
        return total

    assert size_of("mcx_storage_date") == _abi.STORAGE_DATE_DTYPE.itemsize == 352
    assert size_of("mcx_storage_desc") == ctypes.sizeof(_abi.StorageDesc) == 32
    assert size_of("mcx_storage_lsm_date") == _abi.STORAGE_LSM_DATE_DTYPE.itemsize == 56
    assert size_of("mcx_storage_op") == _abi.STORAGE_OP_DTYPE.itemsize == 24
