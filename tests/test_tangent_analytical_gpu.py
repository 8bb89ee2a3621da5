"""Forward-mode sensitivities under the ANALYTICAL scheme on the GPU (csrc/kt_book.hip kt_paths_chol behind mcx_tangent_paths_chol,
driven by mcx.aad.run_with_tangent_book).

  1. the kernel on injected normals: the value image is the path kernel's, the tangent images are a float64 numpy restatement of the
     recursion differentiated by complex step — every model parameter, one and several slots, an odd number of normals, a padded
     last parameter chunk, a partial second block;
  2. the kernel on its own Philox draws: the path kernel's paths, and any split of the path range gives the same bytes;
  3. EULER through the new entry point is mcx_tangent_paths, byte for byte;
  4. refusals by code and wording, with nothing written;
  5. end to end against the reference's autograd (fixtures of tests/analytical_aad_cases.py); the fallback of a book the forward
     pass still cannot take; three emulated ranks."""
import copy
import types

import numpy as np
import pytest
import torch

import analytical_aad_cases as aad_cases
import cases
from mcx import _abi, aad
from mcx._native import McxError
from mcx.plan import SimPlan
from test_oracle_golden import check_lsm_sensitivities
from test_tangent_analytical_host import MODELS, TIMELINE

pytestmark = pytest.mark.gpu
NP = _abi.TANGENT_NP


# ---- descriptors of a bare simulation and the numpy restatement --------------------------------------------------------------------
def _sim_numbers(model, plan, dtype=np.float64):
    """what the path kernel reads of `model` on the sub-step schedule of `plan`: slot parameters, initial state, step constants and
    the closed-form factors (aad._host_descriptors without a book)"""
    slots = np.zeros((plan.n_slots, _abi.SLOT_NPARAM), dtype=dtype)
    for s, sp in enumerate(model._slots()):
        slots[s, :len(sp.params)] = sp.params
    aux = np.zeros(plan.aux.shape, dtype=dtype)
    for k in range(plan.n_steps):
        for s, vals in enumerate(model._step_aux(plan.scheme, float(plan.steps["t1"][k]), float(plan.steps["dt"][k]))):
            aux[k, s, :len(vals)] = vals
    chol = np.array([model._analytic_factor_entries(dt) for dt in plan.chol_dt], dtype=dtype).reshape(plan.chol.shape)
    return dict(slots=slots, init=np.array(model._initial_state(), dtype=dtype), aux=aux, chol=chol)


def _derivatives(model, plan):
    """d (slots, init, aux, chol) / d theta_j for every parameter, by complex step: [..., P] — the driver's own descriptor tangents
    on a bare simulation (a book without atoms)"""
    bare = types.SimpleNamespace(sim_plan=plan, _comp=types.SimpleNamespace(atoms=[], atom_src=[]))
    d0, dd = aad.descriptor_tangents(bare, model, False, mode="complex")
    want = _sim_numbers(model, plan)
    assert all(np.array_equal(d0[k], want[k]) for k in want)
    return dd


def _restated_paths(model, plan, z, j, h):
    """the ANALYTICAL recursion (black_scholes.py:61-67, vasicek.py:76-86 of the reference) at theta_j + i h in complex float64
    numpy on the normals z [n_steps][n_z][n]: [T][D][n] complex — real part the paths, imaginary part / h their tangent"""
    m = copy.deepcopy(model)
    aad._set_complex_step(m, j, h)
    num = _sim_numbers(m, plan, np.complex128)
    n = z.shape[2]
    kinds = [sp.kind for sp in model._slots()]
    offs = np.cumsum([0] + [sp.state_dim for sp in model._slots()])
    state = np.repeat(num["init"][:, None], n, axis=1)
    out = np.zeros((plan.n_dates, plan.n_state, n), dtype=np.complex128)
    for t in range(plan.n_initial_store):
        out[t] = state
    for k in range(plan.n_steps):
        st = plan.steps[k]
        zc = num["chol"][st["chol_idx"]] @ z[k]
        for s, kind in enumerate(kinds):
            c, ax = offs[s], num["aux"][k, s]
            if kind == _abi.MODEL_BS:
                state[c] = state[c] * np.exp(ax[0] + (zc[s] - ax[1]))
            else:
                r, mean = state[c].copy(), num["slots"][s, 2]
                state[c + 1] = state[c + 1] + r * st["dt"]
                state[c] = (mean + (r - mean) * ax[0]) + zc[s]
        if st["store_idx"] >= 0:
            out[st["store_idx"]] = state
    return out


def _chunks(dd, P):
    for c0 in range(0, P, NP):
        sel = list(range(c0, min(c0 + NP, P)))
        yield sel, {k: aad.pad_chunk(v, sel) for k, v in dd.items()}


@pytest.fixture(scope="module")
def sims(hip):
    """per model shape: the model, its plan on [0, 0.25, 1] with two sub-steps (a date at the calibration time, two factors), the
    native simulation and the descriptor derivatives"""
    out = {}
    for name, (build, _) in MODELS.items():
        model = build()
        plan = SimPlan(model, TIMELINE, cases.A, 2)
        assert plan.n_initial_store == 1 and len(plan.chol) == 2 and plan.n_steps == 4
        out[name] = (model, plan, hip.sim_create(plan), _derivatives(model, plan))
    return out


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("name", list(MODELS))
def test_kernel_on_injected_normals(name, n, sims, hip):
    model, plan, sim, dd = sims[name]
    P = len(model.get_model_params())
    # chunks of NP parameters: 3 (one padded chunk), 4 (one full chunk), 7 (two chunks, the last padded), 12 (three full chunks)
    assert P == {"black_scholes": 3, "vasicek": 4, "multi3": 7, "config4": 12}[name] and NP == 4
    z = np.random.default_rng(11).normal(size=(plan.n_steps, plan.n_z, n))
    d_z = hip.from_numpy(z)
    primal = hip.generate_paths(sim, 0, 0, n, inject_z=d_z).cpu().numpy()
    for sel, d in _chunks(dd, P):
        paths, dpaths = hip.tangent_paths_chol(sim, d["slots"], d["init"], d["aux"], d["chol"], 0, 0, n, d_z)
        paths, dpaths = paths.cpu().numpy(), dpaths.cpu().numpy()
        assert np.allclose(paths, primal, rtol=1e-11, atol=1e-13), (name, n, np.abs(paths - primal).max())
        for q in range(NP):
            if q >= len(sel):                                                 # the padding of the last chunk: zero in, zero out
                assert not dpaths[q].any(), (name, n, q)
                continue
            theta = float(model.get_model_params()[sel[q]].detach())
            h = 1e-30 * max(abs(theta), 1e-2)
            ref = _restated_paths(model, plan, z, sel[q], h)
            assert np.allclose(ref.real, primal, rtol=1e-11, atol=1e-13)
            dref = ref.imag / h
            scale = np.abs(dref).max(axis=2, keepdims=True)                   # per (date, state) row
            gap = np.abs(dpaths[q] - dref)
            print(f"{name} n={n} d/d theta_{sel[q]}: worst gap / row scale = {float((gap / np.maximum(scale, 1e-300)).max()):.3e}")
            assert np.all(gap <= 1e-8 * scale), (name, n, sel[q], float((gap / np.maximum(scale, 1e-300)).max()))


# ---- Philox ---------------------------------------------------------------------------------------------------------------------------
def test_kernel_on_philox_draws(sims, hip):
    model, plan, sim, dd = sims["multi3"]
    n, seed = 257, 43
    primal = hip.generate_paths(sim, seed, 0, n).cpu().numpy()
    _, d = next(_chunks(dd, len(model.get_model_params())))
    args = (sim, d["slots"], d["init"], d["aux"], d["chol"], seed)
    paths, dpaths = hip.tangent_paths_chol(*args, 0, n)
    assert np.allclose(paths.cpu().numpy(), primal, rtol=1e-11, atol=1e-13)
    assert float(dpaths.abs().max()) > 0.0 and not bool(torch.isnan(dpaths).any())
    p0, dp0 = hip.tangent_paths_chol(*args, 0, 100)
    p1, dp1 = hip.tangent_paths_chol(*args, 100, 157)
    assert torch.cat([p0, p1], dim=2).cpu().numpy().tobytes() == paths.cpu().numpy().tobytes()
    assert torch.cat([dp0, dp1], dim=3).cpu().numpy().tobytes() == dpaths.cpu().numpy().tobytes()


# ---- EULER through the new entry point ---------------------------------------------------------------------------------------------
def test_euler_through_the_new_entry_is_the_old_one(hip):
    _, model, rm = cases.mixed_cva()
    plan = SimPlan(model, np.linspace(0.0, 2.5, 8), cases.E, 2)
    sim = hip.sim_create(plan)
    rng = np.random.default_rng(3)
    dslot, dinit = rng.normal(0.0, 0.05, (plan.n_slots, _abi.SLOT_NPARAM, NP)), rng.normal(0.0, 0.05, (plan.n_state, NP))
    daux = rng.normal(0.0, 0.05, (plan.n_steps, plan.n_slots, _abi.AUX, NP))
    old = hip.tangent_paths(sim, dslot, dinit, daux, 43, 0, 300)
    new = hip.tangent_paths_chol(sim, dslot, dinit, daux, None, 43, 0, 300)
    assert float(old[1].abs().max()) > 0.0
    for a, b in zip(old, new):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _refused(hip, model, scheme, n=64, dchol="zeros", ld=None):
    """call mcx_tangent_paths_chol on zero derivative tables and sentinel outputs; returns the error after checking that nothing was written"""
    plan = SimPlan(model, TIMELINE, scheme, 1)
    sim = hip.sim_create(plan)
    out = (torch.full((plan.n_dates, plan.n_state, n), 7.0, dtype=torch.float64, device=hip.device),
           torch.full((NP, plan.n_dates, plan.n_state, n), 7.0, dtype=torch.float64, device=hip.device))
    with pytest.raises(McxError) as e:
        hip.tangent_paths_chol(sim, np.zeros((plan.n_slots, _abi.SLOT_NPARAM, NP)), np.zeros((plan.n_state, NP)),
                               np.zeros((plan.n_steps, plan.n_slots, _abi.AUX, NP)),
                               np.zeros((len(plan.chol), plan.n_z, plan.n_z, NP)) if dchol == "zeros" else None, 43, 0, n, out=out, ld=ld)
    hip.synchronize()
    assert bool((out[0] == 7.0).all()) and bool((out[1] == 7.0).all())
    return e.value


def _refused_ld(hip, entry, model, scheme, n=64):
    """mcx_tangent_paths / mcx_tangent_paths_s2f (their wrappers always pass ld = n_paths) as a C caller would call them, with
    ld = n - 1 on zero tables and sentinel outputs; returns the error after checking that nothing was written"""
    plan = SimPlan(model, TIMELINE, scheme, 1)
    sim = hip.sim_create(plan)
    out = (torch.full((plan.n_dates, plan.n_state, n), 7.0, dtype=torch.float64, device=hip.device),
           torch.full((NP, plan.n_dates, plan.n_state, n), 7.0, dtype=torch.float64, device=hip.device))
    tables = [np.zeros((plan.n_slots, _abi.SLOT_NPARAM, NP)), np.zeros((plan.n_state, NP)), np.zeros((plan.n_steps, plan.n_slots, _abi.AUX, NP))]
    if entry != "mcx_tangent_paths":
        tables.append(np.zeros((len(plan.chol), plan.n_z, plan.n_z, NP)))
    with pytest.raises(McxError) as e:
        hip._check(getattr(hip.lib, entry)(hip.h, sim.ptr, *[_abi.ptr(t) for t in tables], 43, 0, n, out[0].data_ptr(), out[1].data_ptr(),
                                           n - 1, None, None), entry)
    hip.synchronize()
    assert bool((out[0] == 7.0).all()) and bool((out[1] == 7.0).all())
    return e.value


def test_refusals(hip):
    from test_hull_white import _hw
    who = "mcx_tangent_paths_chol:"
    for scheme in (cases.E, cases.A):
        e = _refused(hip, cases.s2f_european()[1], scheme)
        assert e.code == _abi.E_NOT_FUSABLE and who in str(e) and f"model kind {_abi.MODEL_S2F}" in str(e), str(e)
    e = _refused(hip, cases.heston()[1], cases.E)
    assert e.code == _abi.E_NOT_FUSABLE and who in str(e) and f"slot 0: model kind {_abi.MODEL_HESTON} has no tangent step" in str(e), str(e)
    e = _refused(hip, _hw(), cases.A)
    assert e.code == _abi.E_NOT_FUSABLE and who in str(e) and f"slot 0: model kind {_abi.MODEL_HW} has no analytic tangent step" in str(e), str(e)
    bs = cases.BlackScholesModel(0.0, 100.0, 0.03, 0.25)
    assert _refused(hip, bs, cases.A, dchol=None).code == -1
    e = _refused(hip, bs, cases.A, ld=63)
    assert e.code == -2 and who in str(e) and "ld < n_paths" in str(e), str(e)
    for entry, model in (("mcx_tangent_paths", bs), ("mcx_tangent_paths_s2f", cases.s2f_european()[1])):
        e = _refused_ld(hip, entry, model, cases.E)
        assert e.code == -2 and f"{entry}: ld < n_paths" in str(e), str(e)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(aad_cases.CASES))
def test_forward_mode_against_reference_autograd(name, hip):
    sc, g = aad_cases.make_controller(name, hip)
    res = sc.run_simulation()
    P = len(sc.model.get_model_params())
    assert sc.timings["tangent"] is True and sc.timings["forward_mode_passes"] == -(-P // NP) and "bumped_passes" not in sc.timings
    check_lsm_sensitivities(sc, g, res)


def test_a_book_with_a_geometric_basket_still_completes_through_bumps(hip):
    ns, model, rm = cases.basket_multi()
    sc = cases.SimulationController(ns, model, rm, 256, 0, 2, cases.A, differentiate=True, backend=hip)
    res = sc.run_simulation()
    assert sc.timings["tangent"] is False and sc.timings["bumped_passes"] == 2 * len(model.get_model_params())
    grads = np.array([[ev for ev in m] for per_ns in res.derivatives for m in per_ns], dtype=np.float64)
    assert np.isfinite(grads).all() and np.abs(grads).max() > 0.0


def test_flexicall_on_three_emulated_ranks_matches_the_single_shard_run(hip):
    from emulated_ranks import run_ranks
    from mcx import _native

    def build(be):
        sc, _ = aad_cases.make_controller("flexicall_aad", be, inject=False)
        sc.materialize = False
        return sc

    def grads(res):
        return [[np.array(m, dtype=np.float64) for m in per_ns] for per_ns in res.derivatives]

    single = build(hip)
    ref = grads(single.run_simulation())
    assert single.timings["tangent"] is True

    def body(sc, rank):
        g = grads(sc.run_simulation())
        assert sc.timings["tangent"] is True
        return g

    out, calls = run_ranks(3, lambda rank: build(_native.HipBackend(0)), body)
    assert calls["all_reduce"] > 0
    for rank, got in enumerate(out):
        for ns_r, ns_g in zip(ref, got):
            for m_r, m_g in zip(ns_r, ns_g):
                assert np.allclose(m_g, m_r, rtol=1e-9, atol=1e-12), (rank, np.abs(m_g - m_r).max())
