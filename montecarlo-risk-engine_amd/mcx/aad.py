"""Sensitivities (`differentiate=True`) without a tape.

The reference puts every model parameter on torch's autograd tape and differentiates each metric value through the whole
simulation (controller/controller.py:609-648).  Here the derivative travels FORWARD with the path: the tangent kernel
(csrc/kt_tangent.hip) carries d state / d theta_j in registers and returns per-path d cashflow / d theta_j, so
d PV / d theta_j = mean_j — identical to the reference's pathwise gradient, including the smoothing it switches on
(`Model.requires_grad`, models/model.py:83-90) and torch's subgradient conventions.

Tangent kernels exist (BASELINE configs 2 and 4) for PV metrics of European options on an Equity under a single
Black-Scholes or Heston model.

Sensitivities through the LSM regression (CVA / PV of stateless books under BS / Vasicek / CIR++ Euler) run in forward mode too:
`run_with_tangent_book` drives csrc/kt_book.hip (dual paths -> dual normal equations -> dual book -> dual CVA).  So do books under
the ANALYTICAL scheme whose slots are Black-Scholes or Vasicek: there the Cholesky factor of the per-dt covariance depends on the
parameters, the models give it in closed form (`Model._analytic_factor_entries`) and mcx_tangent_paths_chol carries its tangent.
With `SimulationController.tangent_heston` a book under a single HestonModel (EULER or QE, no storage) whose metrics go through
exposures or exercise takes the same pass on the dual paths of mcx_tangent_paths_heston (`heston_route`).
With `SimulationController.tangent_wide` a book under 5 to 32 correlated one-factor sub-models takes it on the dual paths of
mcx_tangent_paths_wide (csrc/kt_wide.hip: one block row per slot the chunk's parameters reach; `wide_route`).
With `SimulationController.tangent_hull_white` a book under 1 to 32 one-factor sub-models of which at least one is Hull-White takes it
on the dual paths of mcx_tangent_paths_wide_hw (`hull_white_route`), in passes over the LIVE parameters only: a curve node beyond the
book's horizon reaches no descriptor number, its rows are exact zeros without a pass.
With `SimulationController.tangent_xva` the five records of DVAMetric / BilateralCVAMetric take their tangents from mcx_tangent_xva
(csrc/kt_book.hip kt_xva; `xva_route`, `_scatter_xva`) on whichever of these passes serves the book; without it such a metric bumps.
With `SimulationController.tangent_fva` the three records of FVAMetric take theirs from mcx_tangent_fva (kt_fva, the dual of k4_fva;
`fva_route`, `_scatter_fva`) in the same way; the two flags are independent, and a book that holds both families needs both.

Every other configuration (`run_with_bumps`): sensitivities through the LSM regression — CVA / EPE / PFE greeks, SURVEY §8f
rank 1, reference test `tests/pytests/test_cva_large_netting_set_aad_vs_fd.py` — are computed by CENTRAL DIFFERENCES WITH
COMMON RANDOM NUMBERS: the Philox counters (or the injected draws) are identical in the bumped runs, so the difference
quotient converges to the same pathwise derivative the reference's tape returns (including the dependence of the regression
coefficients on the parameters through the pre-simulation), with O(h^2) truncation and no sampling noise.  It costs 2P + 1
passes of the millisecond-scale hot path and serves what the forward-mode kernels do not cover (exercise products, PFE,
collateral, analytic exposures, the QE scheme, Heston / Hull-White / S2F slots under ANALYTICAL).

Exercise products (American / Bermudan / FlexiCall): the reference's tape has NO gradient through the boolean
`should_exercise` (bermudan_option.py:122-128): its sensitivities hold the exercise policy fixed.  A plain bump would let paths
near the exercise boundary flip their decision and add jump / (2 h N) spikes, so the base run RECORDS every exercise decision
(pre-simulation roll and main simulation, mcx_book_set_exercise_replay) and the bumped pair REPLAYS them; pinned against the
reference's autograd gradients (tests/golden/bermudan_swaption_aad.npz, american_put_aad.npz)."""
from __future__ import annotations

import copy
import ctypes as C
import os
import math
import time
from collections import namedtuple
from operator import itemgetter
from types import SimpleNamespace

import numpy as np

from . import _abi
from .maths.regression import regression_centering
from .metrics.metric import MetricType, XvaMetricType, mean_and_error
from .models.black_scholes import BlackScholesModel
from .models.heston import HestonModel
from .plan import SimPlan, UnsecuredSpec


class TangentOption(C.Structure):
    _fields_ = [("t_idx", C.c_int32), ("netting_set", C.c_int32), ("strike", C.c_double), ("sign", C.c_double),
                ("numeraire", C.c_double), ("dnum_drate", C.c_double)]


def _wide_model(model) -> bool:
    """more than MCX_MAX_SLOTS sub-models: the wide path kernel serves it, no fused kernel does, and in forward mode only
    mcx_tangent_paths_wide (wide_route)"""
    return len(model._slots()) > _abi.MAX_SLOTS


def _check_supported(sc):
    from .products.equity import Equity
    from .products.european_option import EuropeanOption
    if _wide_model(sc.model):
        raise NotImplementedError("differentiate=True: a wide model (more than MCX_MAX_SLOTS sub-models) has no tangent kernels")
    if not isinstance(sc.model, (BlackScholesModel, HestonModel)):
        raise NotImplementedError("differentiate=True: tangent kernels exist for a single BlackScholesModel or HestonModel")
    if any(m.metric_type != MetricType.PV or not m._native for m in sc.risk_metrics.metrics):
        raise NotImplementedError("differentiate=True: only PV metrics are differentiated in this round "
                                  "(exposure / CVA sensitivities go through the LSM regression: SURVEY §8f rank 1)")
    for p in sc.products:
        if not isinstance(p, EuropeanOption) or not isinstance(p.underlying, Equity):
            raise NotImplementedError("differentiate=True: European options on an Equity underlying only")
    if sc.requires_higher_order_derivatives:
        raise NotImplementedError("second-order derivatives are not implemented")
    if any(sc._can_skip_monte_carlo_for_product(p) for p in sc.products):
        raise NotImplementedError("analytically valued products are not Monte-Carlo PVs")
    if len(sc.netting_sets) > _abi.FUSED_MAX_NS:
        raise NotImplementedError(f"differentiate=True: at most {_abi.FUSED_MAX_NS} netting sets")


def run_with_tangents(sc):
    from .parallel import Shard
    _check_supported(sc)
    t0 = time.perf_counter()
    be = sc.backend
    shard = sc.shard_factory()
    model = sc.model
    plan = SimPlan(model, sc.simulation_timeline.numpy(), sc.simulation_scheme, sc.num_steps)
    sim = plan.create_sim(be)
    sc.sim_plan = plan
    tl = {float(t): i for i, t in enumerate(sc.simulation_timeline)}
    rate, t_cal = model._pf(2), model.t0()
    opts = (TangentOption * len(sc.products))()
    for k, p in enumerate(sc.products):
        T = float(p.exercise_date[0])
        num = math.exp(rate * (T - t_cal))
        opts[k].t_idx, opts[k].netting_set = tl[T], sc.product_to_netting_set_idx[k]
        opts[k].strike, opts[k].sign, opts[k].numeraire, opts[k].dnum_drate = p._K, p._sign(), num, (T - t_cal) * num
    off, n_local = shard.split(sc.num_paths_mainsim)
    inject = sc._inject.get("main", (None, None))
    P = len(model.get_model_params())
    cfs, dcfs = be.tangent_european(sim, opts, len(sc.netting_sets), P, 43, off, n_local, inject[0], inject[1])
    sc.last_state.update(cfs=cfs, dcfs=dcfs, paths=None, expo=None)
    results, grads = [], []
    for ns_i in range(len(sc.netting_sets)):
        pv = mean_and_error(shard.all_gather_np(be.reduce_vector(cfs[ns_i]).view(np.float64)))
        g = [mean_and_error(shard.all_gather_np(be.reduce_vector(dcfs[ns_i, j]).view(np.float64)))[0] for j in range(P)]
        results.append([[pv] for _ in sc.risk_metrics.metrics])
        grads.append([[tuple(g)] for _ in sc.risk_metrics.metrics])
    sc.timings = dict(total=time.perf_counter() - t0, tangent=True)
    return sc._package(results, grads, [])


# ---- central differences with common random numbers ---------------------------------------------------------------------
def _leaf_models(model):
    return list(model.models) if hasattr(model, "models") else [model]


def _set_param(model, j: int, value: float):
    """overwrite the j-th entry of `model.get_model_params()` (ModelConfig: concatenation in sub-model order)"""
    import torch
    model._cholesky = {}                       # factors of a covariance matrix depend on the parameters (ANALYTICAL scheme)
    for m in _leaf_models(model):
        m._cholesky = {}
    for m in _leaf_models(model):
        n = len(m.model_params)
        if j < n:
            m.model_params[j] = torch.tensor(float(value), dtype=m.model_params[j].dtype)
            if hasattr(model, "models"):       # ModelConfig keeps the concatenated list
                model.model_params = [p for sub in model.models for p in sub.get_model_params()]
            return
        j -= n
    raise IndexError("parameter index out of range")


def bump_size(theta: float) -> float:
    return 1e-5 * max(abs(theta), 1e-2)


def _clone_controller(sc, model, float32_cache, objects=None, force_wide=False):
    """a controller on the same book under `model`.  objects: (netting_sets, risk_metrics) to build it on — a private deep copy by
    default; the bumped controllers of one differentiation run one after the other and share ONE copy (a run only reassigns the
    regression coefficients it produces; copying the product graph was 12 ms per controller).  force_wide: the clone builds its
    SimPlan with force_wide=True (the base controller of a forward-mode pass on the wide route, for a model of 5 to 8 slots)"""
    import copy
    from .controller.controller import SimulationController
    ns, rm = objects if objects is not None else (copy.deepcopy(sc.netting_sets), copy.deepcopy(sc.risk_metrics))
    clone = SimulationController(ns, model, rm, sc.num_paths_mainsim,
                                 sc.num_paths_presim, sc.num_steps, sc.simulation_scheme, differentiate=False,
                                 regression_function=sc.regression_function, backend=sc.backend, use_mfma=sc.use_mfma)
    for attr in ("seed_offset", "allow_fused", "main_plan", "materialize", "_inject", "date_batched_lsm"):
        setattr(clone, attr, getattr(sc, attr))
    clone.reference_float32_cf_cache = float32_cache
    clone._force_wide_plan = bool(force_wide)
    return clone


def run_with_bumps(sc):
    import copy
    if sc.requires_higher_order_derivatives:
        raise NotImplementedError("second-order derivatives are not implemented")
    t0 = time.perf_counter()
    smoothing = getattr(sc.model, "perform_smoothing", False)      # the reference differentiates the smoothed payoffs
    base = _clone_controller(sc, sc.model, sc.reference_float32_cf_cache)
    # Exercise products: the reference's tape has no gradient through the boolean `should_exercise` (bermudan_option.py:122-128),
    # i.e. its sensitivities hold the exercise policy fixed.  The base run records every exercise decision (pre-simulation roll
    # and main simulation), the bumped runs replay them: no path flips its policy under the bump.
    replay = None
    if any(p.get_num_states() > 1 for p in sc.products) and hasattr(sc.backend, "book_set_exercise_replay"):
        replay = dict(mode=1, pre=None, main=None)
        base.exercise_replay = replay
    res0 = base.run_simulation()
    if replay is not None:
        base.backend.book_set_exercise_replay(base.book, 0, None)
    sc.sim_plan, sc.last_state = base.sim_plan, base.last_state
    theta = [float(p.detach()) for p in sc.model.get_model_params()]
    P = len(theta)
    vals = []                       # [param][sign] -> nested results
    shared = (copy.deepcopy(sc.netting_sets), copy.deepcopy(sc.risk_metrics))      # the bumped controllers' object graph
    for j in range(P):
        h = bump_size(theta[j])
        pair = []
        for sgn in (+1.0, -1.0):
            m = copy.deepcopy(sc.model)
            m.perform_smoothing = smoothing
            for leaf in _leaf_models(m):
                leaf.perform_smoothing = smoothing
            _set_param(m, j, theta[j] + sgn * h)
            # the float32 cashflow cache of the reference's LSM is a rounding artefact: differencing through it would only add
            # noise of size eps_f32 / h, so the bumped pair runs with the float64 cache
            bumped = _clone_controller(sc, m, False, shared)
            if replay is not None:
                bumped.exercise_replay = dict(mode=2, pre=replay["pre"], main=replay["main"])
            pair.append(bumped.run_simulation().results)
            if replay is not None:
                bumped.backend.book_set_exercise_replay(bumped.book, 0, None)
            bumped.release_device_buffers()
        vals.append((pair, h))
    grads = []
    for ns_i, per_metric in enumerate(res0.results):
        gm = []
        for m_i, evals in enumerate(per_metric):
            ge = []
            for e_i in range(len(evals)):
                ge.append(tuple((float(vals[j][0][0][ns_i][m_i][e_i][0]) - float(vals[j][0][1][ns_i][m_i][e_i][0])) / (2.0 * vals[j][1])
                                for j in range(P)))
            gm.append(ge)
        grads.append(gm)
    sc.timings = dict(total=time.perf_counter() - t0, tangent=False, bumped_passes=2 * P)
    return sc._package([[[tuple(v) for v in evals] for evals in per_metric] for per_metric in res0.results], grads, [])


def tangent_kernels_apply(sc) -> bool:
    try:
        _check_supported(sc)
        return True
    except NotImplementedError:
        return False


# ---- forward mode through the exposure path (csrc/kt_book.hip) ---------------------------------------------------------------
class _NoTangentForm(Exception):
    pass


def _host_descriptors(sc, model=None, dtype=np.float64, factor=False):
    """every host-computed number the kernels consume (slot parameters, initial state, per-step tables, atom coefficients) of a
    COMPILED controller, re-evaluated under `model` (default: its own) WITHOUT touching the GPU.  Only the model-dependent
    numbers are recomputed: the per-step tables of the existing sub-step schedule and the closed-form coefficients of the
    existing atoms (requests, events and terms do not depend on the model parameters).  factor: under ANALYTICAL the closed-form factor
    block also for a model whose slots the narrow dual path kernels do not all serve (hull_white_route: a Hull-White slot)."""
    model = sc.model if model is None else model
    sim, comp = sc.sim_plan, sc._comp
    specs = model._slots()
    slots = np.zeros((sim.n_slots, _abi.SLOT_NPARAM), dtype=dtype)
    for s, sp in enumerate(specs):
        slots[s, :len(sp.params)] = sp.params
    aux = np.zeros(sim.aux.shape, dtype=dtype)
    for k in range(sim.n_steps):
        for s, vals in enumerate(model._step_aux(sim.scheme, float(sim.steps["t1"][k]), float(sim.steps["dt"][k]))):
            aux[k, s, :len(vals)] = vals
    atoms = np.zeros((len(comp.atoms), 5), dtype=dtype)
    cols = []
    for q, src in enumerate(comp.atom_src):
        if src is None:
            atoms[q, 0] = comp.atoms[q][2]
            cols.append(-1)
            continue
        co = model._atom(*src)
        atoms[q] = (co.a, co.d, co.b, co.c0, co.c1)
        cols.append(-1 if co.col is None else co.col)
    shape = (tuple(cols), tuple(sp.kind for sp in specs))
    out = dict(slots=slots, init=np.array(model._initial_state(), dtype=dtype), aux=aux, atoms=atoms)
    if hasattr(model, "_cholesky_entries"):          # factors that depend on the parameters (a correlation that is one of them)
        out["chol"] = np.array([model._cholesky_entries(sim.scheme, dt) for dt in sim.chol_dt], dtype=dtype).reshape(len(sim.chol_dt), sim.n_z, sim.n_z)
    elif _analytic_factor_form(model, sim.scheme) or (factor and sim.scheme.name == "ANALYTICAL"):   # ANALYTICAL: the factor of the per-dt covariance (volatilities, mean reversion)
        out["chol"] = np.array([model._analytic_factor_entries(dt) for dt in sim.chol_dt], dtype=dtype).reshape(len(sim.chol_dt), sim.n_z, sim.n_z)
    return out, shape


def _analytic_factor_form(model, scheme) -> bool:
    """does `model` give the ANALYTICAL scheme's Cholesky factor in closed form (Model._analytic_factor_entries), with every slot
    one whose analytic step the dual path kernel has (csrc/kt_book.hip kt_paths: Black-Scholes, Vasicek)?"""
    entries = getattr(model, "_analytic_factor_entries", None)
    if scheme.name != "ANALYTICAL" or entries is None or entries(1.0) is None:
        return False
    return all(sp.kind in (_abi.MODEL_BS, _abi.MODEL_VASICEK) for sp in model._slots())


def _set_complex_step(model, j: int, h: float):
    """evaluate the closed forms at theta_j + i h (Model._pf): j indexes `model.get_model_params()`"""
    for m in _leaf_models(model):
        n = len(m.model_params)
        m._complex_step = [complex(float(p.detach()), h if q == j else 0.0) for q, p in enumerate(m.model_params)]
        j -= n


def _solve_dual(mom: np.ndarray, K: int, shift: float, scale: float, degenerate: bool, n_par: int):
    """coefficients and their tangents in the RAW monomial basis from the dual moments of mcx_tangent_lsm:
    G c = r  =>  dc = G^-1 (dr - dG c)   (what autograd through torch.linalg.lstsq returns at full rank)"""
    m, dm = mom[0], mom[1:1 + n_par]
    n = m[0]
    c, dc = np.zeros(K), np.zeros((n_par, K))
    if n <= 0:
        return c, dc
    if degenerate:
        # all paths share x = x0 (t = calibration date): minimum-norm solution c = v ybar / (v.v), v = [1, x0, .., x0^(K-1)];
        # z = x - x0 is zero in value, its tangent is d x0
        x0 = shift
        ybar, dybar, dx0 = m[2 * K - 1] / n, dm[:, 2 * K - 1] / n, dm[:, 1] / n
        v = np.array([x0 ** k for k in range(K)])
        dv = np.array([k * x0 ** (k - 1) if k > 0 else 0.0 for k in range(K)])
        vv = float(v @ v)
        c = v * (ybar / vv)
        for q in range(n_par):
            dvq = dv * dx0[q]
            dc[q] = dvq * (ybar / vv) + v * (dybar[q] / vv) - v * (ybar * 2.0 * float(v @ dvq) / vv ** 2)
        return c, dc
    idx = np.arange(K)[:, None] + np.arange(K)[None, :]
    G, r = m[idx], m[2 * K - 1:2 * K - 1 + K]
    cz = np.linalg.solve(G, r)
    T = np.zeros((K, K))
    for k in range(K):
        for j in range(k + 1):
            T[j, k] = (scale ** k) * math.comb(k, j) * ((-shift) ** (k - j))
    c = T @ cz
    for q in range(n_par):
        dG, dr = dm[q][idx], dm[q][2 * K - 1:2 * K - 1 + K]
        dc[q] = T @ np.linalg.solve(G, dr - dG @ cz)
    return c, dc


def _solve_dual_states(mom: np.ndarray, K: int, S: int, shift: float, scale: float, degenerate: bool, n_par: int):
    """_solve_dual for the S right-hand sides of an exercise product (moments of mcx_tangent_lsm_step: sums of z^k, then of
    z^k Y_s per state s): c [S][K], dc [n_par][S][K]"""
    c, dc = np.zeros((S, K)), np.zeros((n_par, S, K))
    for s_ in range(S):
        sel = list(range(2 * K - 1)) + list(range(2 * K - 1 + s_ * K, 2 * K - 1 + (s_ + 1) * K))
        cs, dcs = _solve_dual(mom[:, sel], K, shift, scale, degenerate, n_par)
        c[s_], dc[:, s_, :] = cs, dcs
    return c, dc


def stateless_lsm_jobs(plan, x_range, expo_coeff_base, K: int):
    """the (product, regression date) pairs of the products WITHOUT exercise states of one forward-mode pass, in the order the
    per-job loop of run_with_tangent_book visits them.  plan: [(product index, product, regression schedule, [(num atom, x atom)])];
    x_range: {x atom: (min, max)}.  Returns the job table (_abi.TANGENT_LSM_JOB_DTYPE: what mcx_tangent_lsm takes per job) and,
    per job, (offset of its K coefficients, degenerate) for _solve_dual.  Products with states (exercise rights, storages) are
    skipped: their backward induction is sequential per product.  Pure host arithmetic."""
    rows, keep = [], []
    for p_i, p, sched, atoms in plan:
        if p.get_num_states() > 1:
            continue
        pdates = np.asarray([float(t) for t in p.product_timeline])
        for (t_reg, _r0, _r1, _prod_idx, expo_idx), (num, x) in zip(sched, atoms):
            if expo_idx is None:
                continue
            shift, scale, degenerate = regression_centering(x_range, x)
            first = int(np.searchsorted(pdates, t_reg, side="right"))      # cashflows strictly after t_reg (controller.py:323)
            rows.append((p_i, first, num, x, shift, scale))
            keep.append((expo_coeff_base[p_i] + expo_idx * K, degenerate))
    return np.array(rows, dtype=_abi.TANGENT_LSM_JOB_DTYPE), keep


def _batch_tangent_lsm(sc) -> bool:
    """which route the regression of the stateless products takes (SimulationController.batch_tangent_lsm): one
    mcx_tangent_lsm_batch call per parameter chunk, or one mcx_tangent_lsm call per (product, date)"""
    flag = getattr(sc, "batch_tangent_lsm", None)
    if flag is False:
        return False
    able = hasattr(sc.backend, "tangent_lsm_batch")
    if flag is None and len(sc.products) <= 64:
        return False
    if not able:            # the per-job route stops at 64 products: ~3 synchronous round trips per (product, date, chunk)
        raise _NoTangentForm("products")
    return True


def no_tangent_form(e) -> bool:
    """is `e` the library's MCX_E_NOT_FUSABLE: a book the forward-mode kernels have no tangent form for?"""
    return getattr(e, "code", None) == _abi.E_NOT_FUSABLE


# The stages of run_with_tangent_book (DESIGN.md "Forward-mode book pass: the stages of the driver").  _BookPass: what every stage
# of one differentiation reads; _Chunk: one group of <= TANGENT_NP parameters, their indices `sel` and their zero-padded descriptor
# tangents; _Presim: the dual pre-simulation of a chunk and the coefficient images its regression fills; _Images: the main pass.
# dpayoff: tangent_payoffs only; heston: the book's dual paths come from mcx_tangent_paths_heston (heston_route)
# wide: the book's dual paths come from mcx_tangent_paths_wide (wide_route); active: {first parameter of a chunk: its active slots}
_BookPass = namedtuple("_BookPass", "sc base be shard s2f chol batched rows base_coeffs dpayoff heston wide active",
                       defaults=(None, False, False, None))
_Chunk = namedtuple("_Chunk", "sel dslot dinit daux dchol datoms")
_Presim = namedtuple("_Presim", "x_range paths dpaths n coeffs dcoeffs")
_Images = namedtuple("_Images", "paths dpaths cfs expo")


def heston_route(sc) -> bool:
    """Host only: do the book's dual paths come from mcx_tangent_paths_heston (csrc/kt_book.hip kt_paths_heston)?  Only with
    SimulationController.tangent_heston on a backend with the binding, for a single HestonModel (not a ModelConfig with a Heston
    leaf) under EULER or QE, and a book without a storage.  Every other Heston book keeps the route it had."""
    return bool(getattr(sc, "tangent_heston", False)) and hasattr(sc.backend, "tangent_paths_heston") \
        and isinstance(sc.model, HestonModel) and sc.simulation_scheme.name in ("EULER", "QE") \
        and not any(getattr(p, "is_storage", False) for p in sc.products)


TANGENT_MAX_SLOTS = 4          # slots the narrow dual path kernels are instantiated for (csrc/kt_book.hip ktp_paths)


def wide_route(sc) -> bool:
    """Host only: do the book's dual paths come from mcx_tangent_paths_wide (csrc/kt_wide.hip kt_paths_wide: one block row per
    ACTIVE slot)?  Only with SimulationController.tangent_wide on a backend with the binding, for a model of more than
    TANGENT_MAX_SLOTS slots (5 to 8 slots: the pass forces the base controller's plan wide; 9 to 32: it is wide already) whose
    every slot is one-factor with a kind the kernel serves under the scheme — EULER: Black-Scholes, Vasicek, CIR++ (stochastic and
    deterministic); ANALYTICAL: Black-Scholes and Vasicek with the factor in closed form — and a book without a storage.  A
    Hull-White slot makes it False: that book is bumped (a wide one without a wasted base run)."""
    if not getattr(sc, "tangent_wide", False) or not hasattr(sc.backend, "tangent_paths_wide"):
        return False
    slots = sc.model._slots()
    if not TANGENT_MAX_SLOTS < len(slots) <= _abi.WIDE_MAX_SLOTS:
        return False
    scheme = sc.simulation_scheme.name
    if scheme == "EULER":
        kinds = (_abi.MODEL_BS, _abi.MODEL_VASICEK, _abi.MODEL_CIRPP, _abi.MODEL_CIRPP_DET)
    elif scheme == "ANALYTICAL" and _analytic_factor_form(sc.model, sc.simulation_scheme):
        kinds = (_abi.MODEL_BS, _abi.MODEL_VASICEK)
    else:
        return False
    return all(sp.sim_dim == 1 and sp.kind in kinds for sp in slots) \
        and not any(getattr(p, "is_storage", False) for p in sc.products)


_XVA_TYPES = (MetricType.DVA, MetricType.BCVA)


def xva_route(sc) -> bool:
    """Host only: do DVAMetric / BilateralCVAMetric take their tangents from mcx_tangent_xva (csrc/kt_book.hip kt_xva, the dual of
    k4_xva)?  Only with SimulationController.tangent_xva on a backend with the binding, and only for the native metrics (a subclass
    with a host form of its own is evaluated by that form, which has no dual).  Otherwise one such metric sends the whole book to
    bump-and-revalue.  Independent of the path routes: the scatter reads the dual images of a pass, whichever kernel made them."""
    return bool(getattr(sc, "tangent_xva", False)) and hasattr(sc.backend, "tangent_xva") \
        and all(m._native for m in sc.risk_metrics.metrics if m.metric_type in _XVA_TYPES)


def fva_route(sc) -> bool:
    """Host only: does FVAMetric take its tangents from mcx_tangent_fva (csrc/kt_book.hip kt_fva, the dual of k4_fva)?  Only with
    SimulationController.tangent_fva on a backend with the binding, and only for the native metrics, as xva_route.  Otherwise one
    FVAMetric sends the whole book to bump-and-revalue.  Independent of tangent_xva and of the path routes"""
    return bool(getattr(sc, "tangent_fva", False)) and hasattr(sc.backend, "tangent_fva") \
        and all(m._native for m in sc.risk_metrics.metrics if m.metric_type == XvaMetricType.FVA)


def hull_white_route(sc) -> bool:
    """Host only: do the book's dual paths come from mcx_tangent_paths_wide_hw (csrc/kt_wide.hip kt_paths_wide<., true>: the per-slot
    kernel with the two Hull-White dual steps)?  Only with SimulationController.tangent_hull_white on a backend with the binding, for
    a model of 1 to WIDE_MAX_SLOTS slots of which at least one is Hull-White, whose every slot is one-factor with a kind the entry
    serves under the scheme — EULER: Black-Scholes, Vasicek, Hull-White, CIR++ (stochastic and deterministic); ANALYTICAL:
    Black-Scholes, Vasicek and Hull-White with the factor in closed form, in practice a single Hull-White model (ModelConfig
    assembles mixed families for Black-Scholes pairs only) — and a book without a storage.  A model without a Hull-White slot is
    never touched by the flag.  A model of 8 slots or fewer runs its base pass on a forced-wide plan, as on wide_route."""
    if not getattr(sc, "tangent_hull_white", False) or not hasattr(sc.backend, "tangent_paths_wide_hw"):
        return False
    slots = sc.model._slots()
    if not 1 <= len(slots) <= _abi.WIDE_MAX_SLOTS or not any(sp.kind == _abi.MODEL_HW for sp in slots):
        return False
    scheme = sc.simulation_scheme.name
    if scheme == "EULER":
        kinds = (_abi.MODEL_BS, _abi.MODEL_VASICEK, _abi.MODEL_HW, _abi.MODEL_CIRPP, _abi.MODEL_CIRPP_DET)
    elif scheme == "ANALYTICAL":
        entries = getattr(sc.model, "_analytic_factor_entries", None)
        if entries is None or entries(1.0) is None:
            return False
        kinds = (_abi.MODEL_BS, _abi.MODEL_VASICEK, _abi.MODEL_HW)
    else:
        return False
    return all(sp.sim_dim == 1 and sp.kind in kinds for sp in slots) \
        and not any(getattr(p, "is_storage", False) for p in sc.products)


def live_parameters(dd) -> list:
    """Host only: the parameters some descriptor tangent block of `dd` (descriptor_tangents: [...][P]) is non-zero for, ascending.
    Every other parameter reaches no number a kernel reads: its sensitivities are exact zeros without a pass (hull_white_route: the
    curve nodes beyond the book's horizon)"""
    P = next(iter(dd.values())).shape[-1]
    return [j for j in range(P) if any(np.any(v[..., j] != 0) for v in dd.values())]


def active_slots(plan, dslot, dinit, daux, dchol=None) -> list:
    """Host only: the slots mcx_tangent_paths_wide launches a block row for, ascending — slot r is active iff any entry of its dslot
    row, its dinit rows, its daux rows over all sub-steps or (dchol given: ANALYTICAL) row r of dchol over all factors is non-zero.
    plan: anything with the slots' state offsets and dimensions (`slot_states`: [(state_off, state_dim)]), or a SimPlan"""
    states = getattr(plan, "slot_states", None)
    if states is None:
        offs = np.cumsum([0] + [sp.state_dim for sp in plan.model._slots()])
        states = [(int(offs[s]), int(sp.state_dim)) for s, sp in enumerate(plan.model._slots())]
    out = []
    for r, (c, dim) in enumerate(states):
        on = np.any(dslot[r] != 0) or np.any(dinit[c:c + dim] != 0) or np.any(daux[:, r] != 0)
        if not on and dchol is not None:
            on = np.any(dchol[:, r] != 0)
        if on:
            out.append(r)
    return out


def _tangent_book_routes(sc):
    """Host only: every gate that holds before any GPU work, in the order their reasons are reported.  -> (s2f, chol, batched):
    which dual path kernel serves the book, and whether the stateless products' regression is batched.  (The Heston route is
    heston_route: it only widens the scheme gate here.)"""
    if sc.requires_higher_order_derivatives:
        raise _NoTangentForm("second order")
    if _wide_model(sc.model) and not wide_route(sc) and not hull_white_route(sc):
        raise _NoTangentForm("wide model")          # bump-and-revalue; the library would refuse after a wasted base run
    # Schwartz two-factor dual paths serve books that hold a storage; every other book keeps the route it had (no tangent form)
    s2f = hasattr(sc.model, "_cholesky_entries") and hasattr(sc.backend, "tangent_paths_s2f") \
        and all(sp.kind == _abi.MODEL_S2F for sp in sc.model._slots()) \
        and any(getattr(p, "is_storage", False) for p in sc.products)
    # ANALYTICAL: the factor of the per-dt covariance depends on the parameters; mcx_tangent_paths_chol carries its tangent for
    # Black-Scholes and Vasicek slots whose models give it in closed form
    chol = not s2f and hasattr(sc.backend, "tangent_paths_chol") and _analytic_factor_form(sc.model, sc.simulation_scheme)
    if sc.simulation_scheme.name != "EULER" and not (s2f and sc.simulation_scheme.name == "ANALYTICAL") and not chol and not heston_route(sc) \
            and not hull_white_route(sc):
        raise _NoTangentForm("scheme")
    if any(m.metric_type not in _SCATTER or not m._native for m in sc.risk_metrics.metrics):
        raise _NoTangentForm("metric")
    if any(m.metric_type in _XVA_TYPES for m in sc.risk_metrics.metrics) and not xva_route(sc):
        raise _NoTangentForm("metric")
    if any(m.metric_type == XvaMetricType.FVA for m in sc.risk_metrics.metrics) and not fva_route(sc):
        raise _NoTangentForm("metric")
    batched = _batch_tangent_lsm(sc)
    if any(p.get_num_states() > 1 for p in sc.products) and not hasattr(sc.backend, "tangent_lsm_step"):
        raise _NoTangentForm("exercise products")
    if any(sc._can_skip_monte_carlo_for_product(p) for p in sc.products):
        raise _NoTangentForm("analytic shortcuts")
    return s2f, chol, batched


def _descriptors_like(base, model, smoothing, shape0, dtype=np.float64, complex_step=None, bump=None, factor=False):
    """the host descriptors of `base` under a copy of `model` at theta_j + i h (complex_step: (j, h)) or with theta_j replaced
    (bump: (j, value)); the copy must keep the descriptor structure `shape0`"""
    m = copy.deepcopy(model)
    m.perform_smoothing = smoothing
    if complex_step is not None:
        _set_complex_step(m, *complex_step)
    else:
        _set_param(m, *bump)
    ev, shape = _host_descriptors(base, m, dtype=dtype, factor=factor)
    if shape != shape0:
        raise _NoTangentForm("descriptor structure depends on the parameters")
    return ev


def descriptor_tangents(base, model, smoothing, mode=None, factor=False):
    """Host only: (d0, dd), every descriptor block of the compiled controller `base` (_host_descriptors) and its derivative
    [...][P] with respect to the P parameters of `model`.  mode (default: the environment's MCX_DESCRIPTOR_FD, else "complex"):
    "complex": the closed forms are analytic in the parameters, so d f / d theta = Im f(theta + i h) / h with h far below rounding —
    ONE evaluation per parameter, no subtractive cancellation (exact to the last bits); a model whose closed forms are written
    with real-only functions (TypeError) falls back to "4": 4-point central differences with a wide step (truncation O(h^4) ~
    1e-12, rounding eps/h ~ 1e-13 relative).  Anything else: the 2-point formula (h = 1e-6 left 1e-5 relative noise on
    d CVA / d sigma_cir: CIR++ sensitivities are small residuals of large cancelling terms).  factor: _host_descriptors'."""
    d0, shape0 = _host_descriptors(base, model, factor=factor)
    theta = [float(p.detach()) for p in model.get_model_params()]
    dd = {k: np.zeros(v.shape + (len(theta),)) for k, v in d0.items()}
    mode = os.environ.get("MCX_DESCRIPTOR_FD", "complex") if mode is None else mode
    if mode == "complex":
        try:
            for j, th in enumerate(theta):
                h = 1e-30 * max(abs(th), 1e-2)
                ev = _descriptors_like(base, model, smoothing, shape0, np.complex128, complex_step=(j, h), factor=factor)
                for k in dd:
                    dd[k][..., j] = ev[k].imag / h
            return d0, dd
        except TypeError:
            mode = "4"
    four_point = mode == "4"
    for j, th in enumerate(theta):
        h = (1e-3 if four_point else 1e-4) * max(abs(th), 1e-2)
        ev = {mult: _descriptors_like(base, model, smoothing, shape0, bump=(j, th + mult * h), factor=factor)
              for mult in ((1, -1, 2, -2) if four_point else (1, -1))}
        for k in dd:
            if four_point:
                dd[k][..., j] = (8.0 * (ev[1][k] - ev[-1][k]) - (ev[2][k] - ev[-2][k])) / (12.0 * h)
            else:
                dd[k][..., j] = (ev[1][k] - ev[-1][k]) / (2.0 * h)
    return d0, dd


def payoff_number_tangent(product, model, smoothing=False):
    """Host only: d product._payoff_number / d theta, [P] — differentiated like every other descriptor number: ONE complex-step
    evaluation per parameter where the closed form is complex-safe (it returns a complex number at theta_j + i h), otherwise the
    4-point central differences of descriptor_tangents' fallback (real-only closed forms: the normal CDF of the geometric price)"""
    theta = [float(p.detach()) for p in model.get_model_params()]
    out = np.zeros(len(theta))

    def at(**kw):
        m = copy.deepcopy(model)
        m.perform_smoothing = smoothing
        if "step" in kw:
            _set_complex_step(m, *kw["step"])
        else:
            _set_param(m, *kw["bump"])
        return product._payoff_number(m)

    for j, th in enumerate(theta):
        h = 1e-30 * max(abs(th), 1e-2)
        v = at(step=(j, h))
        if isinstance(v, complex):
            out[j] = v.imag / h
            continue
        h = 1e-3 * max(abs(th), 1e-2)
        f = {mult: float(at(bump=(j, th + mult * h))) for mult in (1, -1, 2, -2)}
        out[j] = (8.0 * (f[1] - f[-1]) - (f[2] - f[-2])) / (12.0 * h)
    return out


def payoff_tangents(base, model, smoothing=False):
    """Host only: [n_events][P], row q = the derivative of the one host-computed payoff number of event q of the compiled
    controller `base` (mode 2: the closed-form geometric price in aux[1]; mode 5: the bridge constant parked at coeff_off); zero
    in every other row.  What mcx_book_set_payoff_tangents takes, P columns wide (pad_chunk cuts it per pass)"""
    ev, prods = base.book_plan.events, base.book_plan.products
    out = np.zeros((len(ev), len(model.get_model_params())))
    for p_i, p in enumerate(base.products):
        row = None
        # a product's payoff event stands twice in the book: among the events of the main pass and among its cash events (LSM)
        for q in [*range(int(prods["ev_begin"][p_i]), int(prods["ev_end"][p_i])), *range(int(prods["cf_begin"][p_i]), int(prods["cf_end"][p_i]))]:
            if ev["kind"][q] == _abi.EV_OPTION and ev["aux"][q][0] in (2.0, 5.0):
                if p._payoff_number(model) is None:
                    raise _NoTangentForm("payoff number")
                if row is None:
                    row = payoff_number_tangent(p, model, smoothing)
                out[q] = row
    return out


def payoff_forms_armed(sc, be) -> bool:
    """does this differentiation arm the book's dual payoff forms?  SimulationController.tangent_payoffs on a backend with the
    entry point — and no storage in the book: the payoff forms next to a storage's dual walk have not been compared with anything,
    so such a book keeps the library's refusal, and with it the NotImplementedError of storage books"""
    return bool(getattr(sc, "tangent_payoffs", False)) and hasattr(be, "book_set_payoff_tangents") \
        and not any(getattr(p, "is_storage", False) for p in sc.products) \
        and not heston_route(sc) and not wide_route(sc) and not hull_white_route(sc)      # the payoff forms on Heston / wide / Hull-White dual paths: not compared either


def pad_chunk(a, sel):
    """the columns `sel` of the trailing parameter axis of `a`, zero-padded to TANGENT_NP columns (what one dual pass carries)"""
    return np.ascontiguousarray(np.concatenate([a[..., sel], np.zeros(a.shape[:-1] + (_abi.TANGENT_NP - len(sel),))], axis=-1))


def _parameter_chunk(ctx, dd, sel):
    """the padded descriptor tangents of the parameters `sel`; the atoms' go to the device, the factors' only where a route reads them"""
    dchol = pad_chunk(dd["chol"], sel) if ctx.s2f or ctx.chol or ctx.heston or (ctx.wide and "chol" in dd) else None
    return _Chunk(sel, pad_chunk(dd["slots"], sel), pad_chunk(dd["init"], sel), pad_chunk(dd["aux"], sel), dchol,
                  ctx.be.from_numpy(pad_chunk(dd["atoms"], sel)))


def _dual_paths(ctx, chunk, seed, off, n, inject_z, inject_u=None):
    """GPU: (paths, dpaths) of n paths from path `off` on, through the dual path kernel of the book's route.  inject_u: the injected
    uniforms of the same simulation (pre-simulation or main), which only the Heston QE step consumes"""
    be, sim, c = ctx.be, ctx.base._sim, chunk
    if ctx.wide:                              # (pre-simulation and main pass of a chunk have the same active slots)
        entry = be.tangent_paths_wide_hw if hull_white_route(ctx.sc) else be.tangent_paths_wide
        paths, dpaths, ctx.active[c.sel[0]] = entry(sim, c.dslot, c.dinit, c.daux, c.dchol, seed, off, n, inject_z)
        return paths, dpaths
    if ctx.heston:
        return be.tangent_paths_heston(sim, c.dslot, c.dinit, c.daux, c.dchol, seed, off, n, inject_z, inject_u)
    if ctx.s2f:
        return be.tangent_paths_s2f(sim, c.dslot, c.dinit, c.daux, c.dchol, seed, off, n, inject_z)
    if ctx.chol:
        return be.tangent_paths_chol(sim, c.dslot, c.dinit, c.daux, c.dchol, seed, off, n, inject_z)
    return be.tangent_paths(sim, c.dslot, c.dinit, c.daux, seed, off, n, inject_z)


def _regress_dates(ctx, job, pre, moments, rolls: bool):
    """Host: the per-date loop the three per-product routes share.  moments(entry, num, x, shift, scale) -> the dual moments of one
    schedule entry summed over all ranks.  rolls: the product carries a cashflow cache backwards, so every date is asked and the
    coefficients stay those of the base run's policy; otherwise only the dates with an exposure row are asked and their
    coefficients are written too.  The [S][K] coefficient tangents of the exposure rows go into the images of `pre`."""
    p_i, p, sched, atoms = job
    S, K, NP = p.get_num_states(), ctx.base.book_plan.n_basis, _abi.TANGENT_NP
    for entry, (num, x) in zip(sched, atoms):
        expo_idx = entry[4]
        if expo_idx is None and not rolls:
            continue
        shift, scale, degenerate = regression_centering(pre.x_range, x)
        mom = moments(entry, num, x, shift, scale)
        if expo_idx is None:
            continue
        o = ctx.base._expo_coeff_base[p_i] + expo_idx * S * K
        if rolls:
            dc = _solve_dual_states(mom, K, S, shift, scale, degenerate, NP)[1].reshape(NP, S * K)
        else:
            pre.coeffs[o:o + K], dc = _solve_dual(mom, K, shift, scale, degenerate, NP)
        pre.dcoeffs[o:o + S * K] = dc.T


def _regress_storage(ctx, chunk, job, pre):
    """GPU + collectives: the storage's backward induction in dual numbers (mcx_tangent_storage_lsm_step): every step rolls at most
    one action date from the integer grid states along the base run's policy; old and new cache alternate"""
    p_i, p = job[:2]
    be, S, NP = ctx.be, p.get_num_states(), _abi.TANGENT_NP
    st = ctx.base._storage_handle(p_i)
    W, dW = be.zeros(2, S, pre.n), be.zeros(2, NP, S, pre.n)
    decide = be.from_numpy(pre.coeffs)
    flags = _abi.LSM_F32_CACHE if ctx.base.reference_float32_cf_cache else 0
    halves = [0, 1]                           # (old, new) half of the double-buffered cache

    def moments(entry, num, x, shift, scale):
        _t_reg, r0, r1 = entry[:3]
        if r1 - r0 > 1:
            raise RuntimeError("internal: a storage step rolls at most one action date")
        roll, (old, new) = (r0 if r1 > r0 else -1), halves
        mom = be.tangent_storage_lsm_step(ctx.base.book, st, roll, num, x, shift, scale, chunk.datoms, decide, pre.paths, pre.dpaths,
                                          W[old], dW[old], W[new], dW[new], flags=flags)
        if roll >= 0:
            halves.reverse()
        return ctx.shard.all_reduce_np(mom)
    _regress_dates(ctx, job, pre, moments, rolls=True)


def _regress_exercise(ctx, chunk, job, pre):
    """GPU + collectives: backward induction with the cashflow cache of every hypothetical state rolled in place, in dual numbers,
    along the frozen policy (mcx_tangent_lsm_step); the coefficient tangents of the exposure rows feed the main pass"""
    p_i, p = job[:2]
    be, S = ctx.be, p.get_num_states()
    W, dW = be.zeros(S, pre.n), be.zeros(_abi.TANGENT_NP, S, pre.n)

    def moments(entry, num, x, shift, scale):
        return ctx.shard.all_reduce_np(be.tangent_lsm_step(ctx.base.book, p_i, entry[1], entry[2], num, x, shift, scale, chunk.datoms,
                                                           pre.paths, pre.dpaths, W, dW))
    _regress_dates(ctx, job, pre, moments, rolls=True)


def _regress_stateless(ctx, chunk, job, pre):
    """GPU + collectives: one mcx_tangent_lsm call per regression date of a product without exercise states"""
    p_i, p = job[:2]
    pdates = np.asarray([float(t) for t in p.product_timeline])

    def moments(entry, num, x, shift, scale):
        first = int(np.searchsorted(pdates, entry[0], side="right"))      # cashflows strictly after t_reg (controller.py:323)
        return ctx.shard.all_reduce_np(ctx.be.tangent_lsm(ctx.base.book, p_i, first, num, x, shift, scale, chunk.datoms, pre.paths,
                                                          pre.dpaths))
    _regress_dates(ctx, job, pre, moments, rolls=False)


def _regress_batched(ctx, chunk, plan, pre) -> int:
    """GPU + collectives: the stateless products' (product, date) pairs in one library call and one collective for the whole moment
    block; their coefficient slots are disjoint from those of the products with states.  -> the number of pairs"""
    K, NP = ctx.base.book_plan.n_basis, _abi.TANGENT_NP
    table, keep = stateless_lsm_jobs(plan, pre.x_range, ctx.base._expo_coeff_base, K)         # (centred there, once per pair)
    if len(table):
        moments = ctx.shard.all_reduce_np(ctx.be.tangent_lsm_batch(ctx.base.book, table, chunk.datoms, pre.paths, pre.dpaths))
        for job, mom, (o, degenerate) in zip(table, moments, keep):
            pre.coeffs[o:o + K], dc = _solve_dual(mom, K, float(job["shift"]), float(job["scale"]), degenerate, NP)
            pre.dcoeffs[o:o + K] = dc.T
    return len(table)


def _regress_chunk(ctx, chunk, plan):
    """GPU + collectives: dual pre-simulation and regression of one chunk.  -> (coeffs, dcoeffs [n_coeffs][NP], pairs batched):
    the book's coefficient image and its tangents, products in ascending index"""
    sc, base = ctx.sc, ctx.base
    n_coeffs = len(base.book_plan.coeffs)
    coeffs, dcoeffs = np.zeros(max(n_coeffs, 1)), np.zeros((max(n_coeffs, 1), _abi.TANGENT_NP))
    if ctx.base_coeffs is not None:
        # exercise decisions are taken from the PRIMAL coefficients of the base run (the reference's tape has no gradient through
        # `should_exercise`, bermudan_option.py:122-128): every row starts from them, the exposure rows get their tangents below
        coeffs[:n_coeffs] = ctx.base_coeffs
    if not plan:
        return coeffs, dcoeffs, 0
    off, n_pre = ctx.shard.split(sc.num_paths_presim)
    paths, dpaths = _dual_paths(ctx, chunk, 42 + sc.seed_offset, off, n_pre, *sc._inject.get("pre", (None, None)))
    if ctx.dpayoff is not None:               # the bridge uniforms of the pre-simulation's paths (controller._perform_regression)
        base._set_bridge_rng(42 + sc.seed_offset, off, "bridge_pre")
    pre = _Presim(base._explanatory_ranges(ctx.shard, plan, paths), paths, dpaths, n_pre, coeffs, dcoeffs)
    for job in plan:
        if job[0] in base._storage_meta:
            _regress_storage(ctx, chunk, job, pre)
        elif job[1].get_num_states() > 1:
            _regress_exercise(ctx, chunk, job, pre)
        elif not ctx.batched:
            _regress_stateless(ctx, chunk, job, pre)
    n_pairs = _regress_batched(ctx, chunk, plan, pre) if ctx.batched else 0
    return coeffs, dcoeffs, n_pairs


def _bs_exposure_slots(base, sc, sel):
    """Host only: [n_events][2] — for the analytic Black-Scholes exposure events (EV_EXPO_BS) the tangent slot of this pass that
    is their sigma / their rate, -1 where the chunk `sel` does not hold it and in every other row; None without such events"""
    ev_kind = base.book_plan.events["kind"]
    if not (ev_kind == _abi.EV_EXPO_BS).any():
        return None
    ev_param = np.full((len(ev_kind), 2), -1, dtype=np.int32)
    for p_i, p in enumerate(sc.products):
        if not (hasattr(p, "_bs_param_indices") and base._can_use_analytic_exposure_for_product(p)):
            continue
        _i_s, i_v, i_r = p._bs_param_indices(sc.model)
        b0, b1 = int(base.book_plan.products["ev_begin"][p_i]), int(base.book_plan.products["ev_end"][p_i])
        rows_bs = np.arange(b0, b1)[ev_kind[b0:b1] == _abi.EV_EXPO_BS]
        ev_param[rows_bs, 0] = sel.index(i_v) if i_v in sel else -1
        ev_param[rows_bs, 1] = sel.index(i_r) if i_r in sel else -1
    return ev_param


def _main_dual_pass(ctx, chunk, coeffs, dcoeffs):
    """GPU: dual main simulation and dual book of one chunk -> _Images (cashflow and exposure images [1 + NP][...])"""
    sc, base, be = ctx.sc, ctx.base, ctx.be
    off, n_main = ctx.shard.split(sc.num_paths_mainsim)
    paths, dpaths = _dual_paths(ctx, chunk, 43 + sc.seed_offset, off, n_main, *sc._inject.get("main", (None, None)))
    if ctx.dpayoff is not None:               # back to the main simulation's bridge uniforms: the seed and path range of these paths
        base._set_bridge_rng(43 + sc.seed_offset, off, "bridge_main")
    ev_param = _bs_exposure_slots(base, sc, chunk.sel)
    d_coeffs, d_dcoeffs = be.from_numpy(coeffs), be.from_numpy(dcoeffs)
    cfs, expo = be.tangent_eval(base.book, chunk.datoms, d_coeffs, d_dcoeffs, paths, dpaths, ev_param)
    for p_i in base._storage_meta:            # a storage owns no events: its dual walk adds to the images just written
        be.tangent_storage_eval(base.book, base._storage_handle(p_i), base._storage_ops(p_i), chunk.datoms, d_coeffs, d_dcoeffs, paths,
                                dpaths, cfs, expo)
    return _Images(paths, dpaths, cfs, expo)


# ---- metric tangents: one function per metric family, writing out[eval][param] for the parameters of the chunk ------------------------
def _mean_over_paths(ctx, vec):
    return mean_and_error(ctx.shard.all_gather_np(ctx.be.reduce_vector(vec).view(np.float64)))[0]


def _scatter_pv(ctx, chunk, ns, m_i, m, img, out):
    for q, j in enumerate(chunk.sel):
        out[0][j] = _mean_over_paths(ctx, img.cfs[1 + q, ns.i])


def _scatter_profile(ctx, chunk, ns, m_i, m, img, out):
    """EPE / ENE per exposure date, CE (positive part of the first exposure date, ce_metric.py), EEPE (plain time average of the EE
    profile, eepe_metric.py) from ONE profile tangent per netting set and chunk: [dates][2][NP] means of 1[u>0] du / 1[u<0] du"""
    if ns.prof is None:
        ns.prof = ctx.shard.all_reduce_np(ctx.be.tangent_profiles(ctx.rows, ns.set.threshold, img.expo, ns.i, ns.delayed, ns.coll)) \
            / float(ctx.sc.num_paths_mainsim)
    for q, j in enumerate(chunk.sel):
        if m.metric_type == MetricType.CE:
            out[0][j] = float(ns.prof[0, 0, q])
        elif m.metric_type == MetricType.EEPE:
            out[0][j] = float(ns.prof[:, 0, q].mean())
        else:
            side = 0 if m.metric_type == MetricType.EPE else 1
            for e_i in range(len(out)):
                out[e_i][j] = float(ns.prof[e_i, side, q])


def _scatter_pfe(ctx, chunk, ns, m_i, m, img, out):
    """the tangent of the path that realises the exact order statistic (the reference differentiates through torch.sort): radix
    select on the primal image, then the first path carrying that value"""
    sc, be, shard = ctx.sc, ctx.be, ctx.shard
    unsec = UnsecuredSpec(ctx.rows, ns.delayed, ns.set.threshold, ns.coll)
    target = ctx.base._select_order_stats(shard, unsec, img.expo[0, ns.i], [m.q_index(sc.num_paths_mainsim)])[:, 0]
    pick = be.tangent_pick(ctx.rows, ns.set.threshold, target, img.expo, ns.i, ns.delayed, ns.coll)
    pick[:, 0] = np.where(pick[:, 0] >= 0, pick[:, 0] + shard.split(sc.num_paths_mainsim)[0], np.inf)          # global path index
    allp = shard.all_gather_np(pick)                                          # [world][dates][1+NP]
    win = np.argmin(allp[:, :, 0], axis=0)
    for e_i in range(len(out)):
        for q, j in enumerate(chunk.sel):
            out[e_i][j] = float(allp[win[e_i], e_i, 1 + q])


def _scatter_cva(ctx, chunk, ns, m_i, m, img, out):
    if ns.set.counterparty_id is not None and m.counterparty_id != ns.set.counterparty_id:
        return
    surv, cond = ctx.base._cva_atoms[m_i]
    cva = ctx.be.tangent_cva(ctx.base.book, chunk.datoms, ctx.rows, surv, cond, ns.set.threshold, m.recovery_rate, img.expo, ns.i,
                             img.paths, img.dpaths, ns.delayed, ns.coll)
    for q, j in enumerate(chunk.sel):
        out[0][j] = _mean_over_paths(ctx, cva[1 + q])


def _scatter_xva(ctx, chunk, ns, m_i, m, img, out):
    """DVAMetric / BilateralCVAMetric: the five records (cva, dva, cva_ftd, dva_ftd, bcva) with their tangents from ONE
    mcx_tangent_xva launch and ONE collective of its 25 sums.  The netting set's counterparty gates the bilateral metric as it gates
    CVAMetric (a gated set keeps its zero rows, nothing is launched); the own name never gates, and DVAMetric has no counterparty"""
    if m.metric_type == MetricType.BCVA and ns.set.counterparty_id is not None and m.counterparty_id != ns.set.counterparty_id:
        return
    (cp_atoms, cp_recovery), (own_atoms, own_recovery) = ctx.base._xva_atoms[m_i]
    sums = ctx.be.tangent_xva(ctx.base.book, chunk.datoms, ctx.rows, cp_atoms, cp_recovery, own_atoms, own_recovery, ns.set.threshold,
                              img.expo, ns.i, img.paths, img.dpaths, ns.delayed, ns.coll)
    mean = ctx.shard.all_reduce_np(sums) / float(ctx.sc.num_paths_mainsim)
    records = range(5) if m.metric_type == MetricType.BCVA else (1,)          # BilateralCVAMetric.EVALUATIONS order; dva alone
    for e_i, r in enumerate(records):
        for q, j in enumerate(chunk.sel):
            out[e_i][j] = float(mean[r, 1 + q])


def _scatter_fva(ctx, chunk, ns, m_i, m, img, out):
    """FVAMetric: the three records (fca, fba, fva) with their tangents from ONE mcx_tangent_fva launch and ONE collective of its 15
    sums.  Gated as the primal metric (controller.py): only by a counterparty the metric names (None applies to every set) against a
    set that has one; a gated set keeps its zero rows, nothing is launched.  The own name never gates.  The funding weights are
    constants of the model parameters"""
    if ns.set.counterparty_id is not None and m.counterparty_id is not None and m.counterparty_id != ns.set.counterparty_id:
        return
    cp_surv, own_surv = ctx.base._fva_atoms[m_i]
    sums = ctx.be.tangent_fva(ctx.base.book, chunk.datoms, ctx.rows, cp_surv, own_surv, m.w_borrow, m.w_lend, ns.set.threshold,
                              img.expo, ns.i, img.paths, img.dpaths, ns.delayed, ns.coll)
    mean = ctx.shard.all_reduce_np(sums) / float(ctx.sc.num_paths_mainsim)
    for e_i in range(3):                                                      # FVAMetric.EVALUATIONS order
        for q, j in enumerate(chunk.sel):
            out[e_i][j] = float(mean[e_i, 1 + q])


_SCATTER = {MetricType.PV: _scatter_pv, MetricType.CVA: _scatter_cva, MetricType.PFE: _scatter_pfe, MetricType.EPE: _scatter_profile,
            MetricType.ENE: _scatter_profile, MetricType.CE: _scatter_profile, MetricType.EEPE: _scatter_profile,
            MetricType.DVA: _scatter_xva, MetricType.BCVA: _scatter_xva, XvaMetricType.FVA: _scatter_fva}


def _scatter_metric_tangents(ctx, chunk, img, grads):
    """GPU + collectives: the chunk's columns of grads[ns][metric][eval][param], every metric by the function of its family"""
    for ns_i, ns in enumerate(ctx.sc.netting_sets):
        coll = ns.is_collateralized()
        delayed = ctx.base.netting_set_delayed_exposure_indices[ns_i].numpy().astype(np.int32) if coll else None
        view = SimpleNamespace(i=ns_i, set=ns, coll=coll, delayed=delayed, prof=None)
        for m_i, m in enumerate(ctx.sc.risk_metrics.metrics):
            _SCATTER[m.metric_type](ctx, chunk, view, m_i, m, img, grads[ns_i][m_i])


def run_with_tangent_book(sc):
    """d PV / d theta and d CVA / d theta in forward mode through pre-simulation, regression and main simulation."""
    s2f, chol, batched = _tangent_book_routes(sc)
    t0 = time.perf_counter()
    be, shard = sc.backend, sc.shard_factory()
    NP = _abi.TANGENT_NP
    # the wide route: a model of 5 to 8 slots has no narrow dual path kernel, so the base controller's plan is forced wide (the
    # paths are the narrow kernel's bit for bit, but the book then runs unfused); a model of more than 8 slots is wide already
    # the Hull-White route is the wide route on mcx_tangent_paths_wide_hw, from one slot on, in passes over the live parameters only
    hw = hull_white_route(sc)
    wide = wide_route(sc) or hw
    base = _clone_controller(sc, sc.model, sc.reference_float32_cf_cache, force_wide=wide and not _wide_model(sc.model))
    res0 = base.run_simulation()
    if base.book_plan.n_basis > 4:
        raise _NoTangentForm("basis")
    # `base` is compiled: its sub-step schedule and atoms are re-evaluated under the bumped models
    _d0, dd = descriptor_tangents(base, sc.model, getattr(sc.model, "perform_smoothing", False), factor=hw)
    t_desc = time.perf_counter() - t0
    t_pre = t_main = 0.0
    P, n_coeffs = len(sc.model.get_model_params()), len(base.book_plan.coeffs)
    grads = [[[[0.0] * P for _ in evals] for evals in res0.results[0]] for _ in sc.netting_sets]     # [ns][metric][eval][param]
    jobs, storage_jobs = base._regression_plan()
    plan = sorted(jobs + storage_jobs, key=itemgetter(0))                    # the coefficient images are filled in product order
    has_exercise = any(p.get_num_states() > 1 for p in sc.products)
    base_coeffs = np.asarray(be.book_get_coeffs(base.book), dtype=np.float64)[:n_coeffs] if (has_exercise and n_coeffs) else None
    rows = base.metric_exposure_indices.numpy().astype(np.int32) if sc.risk_metrics.requires_exposure_profiles() else np.zeros(0, dtype=np.int32)
    # SimulationController.tangent_payoffs: the payoff modes 1-5 in dual numbers.  The book is armed per chunk with the tangents of
    # the events' host-computed numbers and disarmed at the end, also on an exception; without the flag (or the entry point) it is
    # never armed, the library refuses such a book and the caller falls back to bump-and-revalue (payoff_forms_armed)
    dpayoff = None
    if payoff_forms_armed(sc, be):
        dpayoff = payoff_tangents(base, sc.model, getattr(sc.model, "perform_smoothing", False))
    ctx = _BookPass(sc, base, be, shard, s2f, chol, batched, rows, base_coeffs, dpayoff, heston_route(sc), wide, {})
    n_batched = 0
    # a parameter no descriptor number depends on (a Hull-White curve node beyond the horizon) keeps its zero rows without a pass
    todo = live_parameters(dd) if hw else list(range(P))
    chunks = [todo[c0:c0 + NP] for c0 in range(0, len(todo), NP)]
    try:
        for sel in chunks:
            chunk = _parameter_chunk(ctx, dd, sel)
            if dpayoff is not None:
                be.book_set_payoff_tangents(base.book, be.from_numpy(pad_chunk(dpayoff, chunk.sel)))
            t1 = time.perf_counter()
            coeffs, dcoeffs, n_pairs = _regress_chunk(ctx, chunk, plan)
            n_batched += n_pairs
            be.synchronize()
            t2 = time.perf_counter()
            t_pre += t2 - t1
            img = _main_dual_pass(ctx, chunk, coeffs, dcoeffs)
            _scatter_metric_tangents(ctx, chunk, img, grads)
            del img                                                           # the large dual tensors go before the next chunk's
            be.synchronize()
            t_main += time.perf_counter() - t2
    finally:
        if dpayoff is not None:
            be.book_set_payoff_tangents(base.book, None)
    sc.sim_plan, sc.last_state = base.sim_plan, base.last_state
    sc.timings = dict(total=time.perf_counter() - t0, tangent=True, forward_mode_passes=len(chunks),
                      base_run_and_descriptor_derivatives=t_desc, presim_and_regression=t_pre, main=t_main,
                      batched_lsm_jobs=n_batched)
    if wide:
        sc.timings["wide_active_slots"] = [ctx.active[sel[0]] for sel in chunks]
    if hw:
        sc.timings["dead_parameters"] = sorted(set(range(P)) - set(todo))
    g = [[[tuple(ev) for ev in per_metric] for per_metric in per_ns] for per_ns in grads]
    return sc._package([[[tuple(v) for v in evals] for evals in per_metric] for per_metric in res0.results], g, [])


# ---- analytically evaluated PV metrics: autograd on the closed form (host scalars, no simulation) --------------------------------
def analytic_controller(sc) -> bool:
    return bool(sc.products) and all(sc._can_skip_monte_carlo_for_product(p) and hasattr(p, "compute_pv_analytically_torch")
                                     for p in sc.products)


def run_analytic_with_autograd(sc):
    """every product is valued by its closed form (PVMetric(ANALYTICAL)): first and, on request, second derivatives come from
    torch.autograd on that closed form, as in the reference (controller.py:609-648; tests/pytests/test_european_option_hessian.py)"""
    import torch
    t0 = time.perf_counter()
    theta = [torch.tensor(float(p.detach()), dtype=torch.float64, requires_grad=True) for p in sc.model.get_model_params()]
    P = len(theta)
    results, grads, hess = [], [], []
    for ns_i, ns in enumerate(sc.netting_sets):
        value = sum(p.compute_pv_analytically_torch(sc.model, theta) for p in ns.products)
        g = torch.autograd.grad(value, theta, create_graph=sc.requires_higher_order_derivatives, allow_unused=True)
        g = [torch.zeros((), dtype=torch.float64) if x is None else x for x in g]
        row = tuple(float(x.detach()) for x in g)
        H = None
        if sc.requires_higher_order_derivatives:
            H = []
            for x in g:
                if x.requires_grad:
                    hx = torch.autograd.grad(x, theta, retain_graph=True, allow_unused=True)
                    H.append(tuple(0.0 if y is None else float(y) for y in hx))
                else:
                    H.append(tuple(0.0 for _ in range(P)))
        results.append([[(float(value.detach()), 0.0)] for _ in sc.risk_metrics.metrics])
        grads.append([[row] for _ in sc.risk_metrics.metrics])
        hess.append([[tuple(H)] if H is not None else [] for _ in sc.risk_metrics.metrics])
    sc.timings = dict(total=time.perf_counter() - t0, analytic=True)
    return sc._package(results, grads, hess if sc.requires_higher_order_derivatives else [])


# ---- second-order derivatives of Monte-Carlo metrics (controller.py:253-255, 631-648) --------------------------------------------
def run_second_order(sc):
    """`compute_higher_derivatives()` with Monte-Carlo metrics: the Hessian as central differences, with common random numbers, of
    the first-order sensitivities this module produces (forward-mode kernels where they exist, replayed bumps otherwise):
    H[i][j] = (g_i(theta + h e_j) - g_i(theta - h e_j)) / 2h, 2P first-order runs.

    What it estimates: the derivative of the pathwise gradient INCLUDING the paths that cross a payoff kink under the bump — the
    term that makes a Monte-Carlo gamma non-zero.  The reference differentiates its tape a second time (`torch.autograd.grad` of
    the gradient, controller.py:631-648), which sees d/dx 1[x > 0] = 0 and therefore returns only the smooth part (a
    Black-Scholes call has gamma exactly 0 on its tape); for parameters that enter smoothly the two agree.  The reference's own
    tests request second derivatives of analytically valued PVs only (tests/pytests/test_european_option_hessian.py), served by
    `run_analytic_with_autograd`.  Bump: 1 % of the parameter (the kink term's variance grows like 1 / (N h))."""
    import copy
    from .controller.controller import SimulationController
    t0 = time.perf_counter()
    theta = [float(p.detach()) for p in sc.model.get_model_params()]
    P = len(theta)

    def first_order(model):
        c = SimulationController(copy.deepcopy(sc.netting_sets), model, copy.deepcopy(sc.risk_metrics), sc.num_paths_mainsim,
                                 sc.num_paths_presim, sc.num_steps, sc.simulation_scheme, differentiate=True,
                                 regression_function=sc.regression_function, backend=sc.backend, use_mfma=sc.use_mfma)
        for attr in ("seed_offset", "allow_fused", "main_plan", "materialize", "_inject", "forward_mode"):
            setattr(c, attr, getattr(sc, attr))
        return c, c.run_simulation()

    base, res0 = first_order(sc.model)
    sc.sim_plan, sc.last_state = base.sim_plan, base.last_state
    cols = []                                       # cols[j][ns][metric][eval] = tuple over i of d g_i / d theta_j
    for j in range(P):
        h = 1e-2 * max(abs(theta[j]), 1e-2)
        g = []
        for sgn in (+1.0, -1.0):
            m = copy.deepcopy(sc.model)
            m.perform_smoothing = getattr(sc.model, "perform_smoothing", False)
            for leaf in _leaf_models(m):
                leaf.perform_smoothing = m.perform_smoothing
            _set_param(m, j, theta[j] + sgn * h)
            g.append(first_order(m)[1].derivatives)
        cols.append([[[tuple((float(a) - float(b)) / (2.0 * h) for a, b in zip(ep, em)) for ep, em in zip(mp, mm)]
                      for mp, mm in zip(np_, nm_)] for np_, nm_ in zip(g[0], g[1])])
    higher = [[[tuple(tuple(cols[j][ns_i][m_i][e_i][i] for j in range(P)) for i in range(P))
                for e_i in range(len(res0.derivatives[ns_i][m_i]))]
               for m_i in range(len(res0.derivatives[ns_i]))] for ns_i in range(len(res0.derivatives))]
    sc.timings = dict(total=time.perf_counter() - t0, second_order_by_differences=True, first_order_runs=2 * P + 1)
    return sc._package([[[tuple(v) for v in evals] for evals in per_metric] for per_metric in res0.results],
                       [[[tuple(ev) for ev in per_metric] for per_metric in per_ns] for per_ns in res0.derivatives], higher)
