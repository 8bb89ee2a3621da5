"""The two Hull-White recursions with EXPLICIT tangents in plain numpy, float64 or np.longdouble (helper, not a test).

State [r, log B]; w is the slot's correlated normal, dw its tangent (ANALYTICAL: the factor depends on sigma and a; EULER: 0):

    both        logB' = logB + r dt;                          dlogB' = dlogB + dr dt
    EULER       r' = r + (theta_k - a r) dt + sigma sqrt(dt) w
                dr' = dr + (dtheta_k - da r - a dr) dt + dsigma sqrt(dt) w + sigma sqrt(dt) dw
                theta_k = aux[0] (theta(t1) of the fitted curve), a = p[3], sigma = p[1]
    ANALYTICAL  r' = r E + shift + w;                         dr' = dr E + r dE + dshift + dw
                E = aux[0] = exp(-a dt), shift = aux[1] = theta(t1) (1 - E) / a

written by hand from the formulas of mcx/models/hull_white.py `_step_aux` (no dual-number class, no fused multiply-adds, not the
kernel's evaluation order).  Every other kind, the correlation, the time loop, the yardstick and the chunking are those of
tests/wide_tangent_reference.py: `run` is its `run` with this module's step in front."""
from __future__ import annotations

import types

import numpy as np

import wide_paths_reference as wr
import wide_tangent_reference as wt

LD = np.longdouble
HW = wr.HW


def _step(kind, scheme, T, p, dp, aux, daux, dt, sq, st, dst, w, dw, res):
    if kind != HW:
        return _WIDE_STEP(kind, scheme, T, p, dp, aux, daux, dt, sq, st, dst, w, dw, res)
    col = lambda v: v[:, None]
    r, logB, dr, dlogB = st[0], st[1], dst[0], dst[1]
    logB_n, dlogB_n = logB + r * dt, dlogB + dr * dt
    if scheme == wr.ANALYTICAL:
        E, shift, dE, dshift = aux[0], aux[1], col(daux[0]), col(daux[1])
        return [r * E + shift + w, logB_n], [dr * E + r * dE + dshift + dw, dlogB_n]
    sigma, a, theta, dsigma, da, dtheta = p[1], p[3], aux[0], col(dp[1]), col(dp[3]), col(daux[0])
    rn = r + (theta - a * r) * dt + sigma * sq * w
    drn = dr + (dtheta - da * r - a * dr) * dt + dsigma * sq * w + sigma * sq * dw
    return [rn, logB_n], [drn, dlogB_n]


_WIDE_STEP = wt._step


def run(plan, z, dslot, dinit, daux, dchol=None, dtype=np.float64):
    """wide_tangent_reference.run with the Hull-White step: its loop looks the step up by name at every call"""
    wt._step = _step
    try:
        return wt.run(plan, z, dslot, dinit, daux, dchol, dtype)
    finally:
        wt._step = _WIDE_STEP


def own_rounding(plan, z, dslot, dinit, daux, dchol=None):
    """float64 run against long-double run of the tangent images, floored at n_sub_steps x 2.2e-16 -> (that number, the long-double run)"""
    lo, hi = run(plan, z, dslot, dinit, daux, dchol, np.float64), run(plan, z, dslot, dinit, daux, dchol, LD)
    hi.lo = lo
    return wt.yardstick(lo, hi, z.shape[2], plan.n_steps), hi


def derivative_tables(model, plan) -> dict:
    """d (slots, init, aux[, chol]) / d theta_j of a bare simulation, [..., P]: the driver's descriptor tangents with the factor block
    the Hull-White route asks for under ANALYTICAL.  Host only"""
    from mcx import aad
    bare = types.SimpleNamespace(sim_plan=plan, _comp=types.SimpleNamespace(atoms=[], atom_src=[]))
    return aad.descriptor_tangents(bare, model, False, mode="complex", factor=True)[1]


def hull_white_leaves(model) -> list:
    """[(first parameter index, leaf)] of every Hull-White leaf, in the order of model.get_model_params()"""
    from mcx.models.hull_white import HullWhiteModel
    out, off = [], 0
    for m in (list(model.models) if hasattr(model, "models") else [model]):
        if isinstance(m, HullWhiteModel):
            out.append((off, m))
        off += len(m.model_params)
    return out


def expected_live(model, times, atoms_to=None) -> list:
    """the parameters of the Hull-White leaves that can reach a descriptor number, from the curve's geometry alone: rate, sigma and
    mean reversion; the two nodes (value and slope) of every segment theta(t1) is read on, t1 in `times` (the sub-steps' left ends);
    and, for zero bonds and discount factors up to atoms_to, the value nodes of every segment that meets [0, atoms_to].  A node
    whose weight at the point it is read is exactly 0 (t on a knot: the far node of the segment) does not count."""
    live = []
    for off, leaf in hull_white_leaves(model):
        ts, n = np.asarray(leaf._t), len(leaf._t)
        vals, slopes = set(), set()

        def touch(t, into):
            idx = min(max(int(np.searchsorted(ts, t)) - 1, 0), n - 2)
            w = (t - ts[idx]) / (ts[idx + 1] - ts[idx])
            if w != 1.0:
                into.add(idx)
            if w != 0.0:
                into.add(idx + 1)

        for t in times:
            touch(float(t), vals)
            touch(float(t), slopes)
        if atoms_to is not None:
            for k in [0.0] + [float(x) for x in ts if 0.0 < x < atoms_to] + [float(atoms_to)]:
                touch(k, vals)
        live += [off, off + 1, off + 2] + [off + 3 + i for i in sorted(vals)] + [off + 3 + n + i for i in sorted(slopes)]
    return sorted(live)


# ---- models and books of the Hull-White tangent tests ---------------------------------------------------------------------------------
def hw_model(n_nodes: int = 6, span: float = 2.5, asset_id: str = "rates", k: int = 0):
    """a Hull-White model on n_nodes equidistant curve nodes over [0, span]: a one-year book on the default curve reaches the nodes
    0 .. 2 and leaves 3 .. 5 dead"""
    from mcx.models.hull_white import HullWhiteModel
    ts = np.linspace(0.0, span, n_nodes)
    f = 0.03 + 0.02 * np.sin(ts / (0.8 + 0.1 * k)) + 0.001 * k
    return HullWhiteModel(0.0, float(f[0]), list(f), list(np.gradient(f, ts)), 0.1 + 0.03 * k, 0.01 + 0.0004 * k, asset_id=asset_id,
                          curve_times=list(ts))


def exercise_book(backend, scheme: str, model=None, n_main: int = 512, n_pre: int = 512, num_steps: int = 2):
    """a Bermudan payer swaption (three exercise rights on a one-year semi-annual swap) under a single Hull-White model; PV and EPE on
    three dates; differentiate=True"""
    import cases
    model = hw_model() if model is None else model
    und = cases.InterestRateSwap(0.0, 1.0, 1.0, 0.03, 0.5, 0.5, cases.IRSType.PAYER, model.asset_ids[0])
    berm = cases.BermudanOption(und, [0.25, 0.5, 0.75], 0.0, cases.OptionType.CALL, asset_id=model.asset_ids[0])
    berm.name = "bermudan"
    rm = cases.RiskMetrics([cases.PVMetric(), cases.EPEMetric()], exposure_timeline=np.array([0.0, 0.5, 1.0]))
    return cases.SimulationController([cases.NettingSet(name="book", products=[berm])], model, rm, n_main, n_pre, num_steps,
                                      cases.SimulationScheme[scheme], differentiate=True, backend=backend)


def cva_book(backend, n_main: int = 512, n_pre: int = 512):
    """a payer swap and a bond in one netting set under ModelConfig[Hull-White, CIR++] (EULER); PV, EPE and CVA; differentiate=True"""
    import cases
    cr = cases.CIRPPModel(0.0, "cp", cases.HAZARDS, kappa=0.4, theta=0.03, volatility=0.04, y0=0.03)
    model = cases.ModelConfig([hw_model(), cr], inter_asset_correlation_matrix=np.array([0.3]))
    swap = cases.InterestRateSwap(0.0, 1.0, 1.0, 0.03, 0.5, 0.5, cases.IRSType.PAYER, "rates")
    swap.name = "swap"
    bond = cases.Bond(0.0, 1.0, 0.5, 0.5, True, 0.02, "rates")
    bond.name = "bond"
    ns = [cases.NettingSet(name="ns", products=[swap, bond], counterparty_id="cp")]
    rm = cases.RiskMetrics([cases.PVMetric(), cases.EPEMetric(), cases.CVAMetric("cp", 0.4)], exposure_timeline=np.array([0.0, 0.5, 1.0]))
    return cases.SimulationController(ns, model, rm, n_main, n_pre, 2, cases.E, differentiate=True, backend=backend)


def bond_book(backend, scheme: str = "EULER"):
    """a coupon bond to 1.2 (coupons every 0.4) under a single Hull-White model; PV only; differentiate=True.  Two sub-steps per
    coupon period: the last theta that reaches the PV is theta(0.8), on the segment [0.5, 1.0], and theta(1.0) reads node 2 alone, so
    every curve node a descriptor reads also moves the PV"""
    import cases
    model = hw_model()
    bond = cases.Bond(0.0, 1.2, 1.0, 0.4, True, 0.02, "rates")
    bond.name = "bond"
    rm = cases.RiskMetrics([cases.PVMetric()])
    return cases.SimulationController([cases.NettingSet(name="ns", products=[bond])], model, rm, 256, 256, 2,
                                      cases.SimulationScheme[scheme], differentiate=True, backend=backend)
