"""One sub-step after another of a list of one-factor sub-models in plain numpy, in float64 or np.longdouble (helper, not a test).

A restatement of what the reference project's time loop does for the five kinds a wide model may hold, written from its model
files and in their order of operations — not from the evaluation order of the kernels (no derived step constants, no fused
multiply-adds):

    correlation   corr_randn = z @ L.T                                              models/model.py:46-48
    BS            EULER       S + (r S dt + sigma S sqrt(dt) w)                     black_scholes.py:79-85
                  ANALYTICAL  S exp(r dt + (w - 0.5 dt sigma^2))                    black_scholes.py:61-67
    Vasicek       EULER       r + a (theta - r) dt + sigma sqrt(dt) w               vasicek.py:104-110
                  ANALYTICAL  theta + (r - theta) exp(-a dt) + w                    vasicek.py:76-84
                  both        logB + r dt  (left endpoint)                          vasicek.py:80 / :107
    Hull-White    EULER       r + (theta(t1) - a r) dt + sigma sqrt(dt) w           hull_white.py:104-108
                  ANALYTICAL  r exp(-a dt) + shift + w                              hull_white.py:76-83
                  both        logB + r dt  (left endpoint)
    CIR++         EULER       max(y + kappa (theta - y) dt + sigma sqrt(max(y, 0)) sqrt(dt) w, 1e-12),
                              Lambda + (y + psi(t1)) dt  (left endpoint)            cirpp.py:188-198
    CIR++ det.    any         lambda_mkt(t2),  Lambda + lambda_mkt(t1) dt           cirpp.py:155-172

The inputs are the doubles a kernel gets: the SimPlan tables (dt, sqrt(dt), the factors, the slot parameters, the aux entries that
are values of curves: psi(t1), theta(t1), lambda_mkt, exp(-a dt), r dt, 0.5 dt sigma^2) and the UNCORRELATED normals z.  The store
rule is the engine's (engine.py:46-62): the leading `n_initial_store` dates hold the start state, a sub-step whose store_idx >= 0
stores the state it reached.

`run(..., dtype=np.float64)` against `run(..., dtype=np.longdouble)` measures the restatement's own rounding: tests bound the
device by a multiple of it."""
from __future__ import annotations

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "wide_paths_reference needs an extended-precision long double"

EULER, ANALYTICAL = 0, 2
BS, VASICEK, CIRPP, CIRPP_DET, HW = 1, 3, 4, 5, 6
STATE_DIM = {BS: 1, VASICEK: 2, CIRPP: 2, CIRPP_DET: 2, HW: 2}
FLOOR = 1e-12


def slot_records(plan) -> list[dict]:
    """(kind, state_off, p[8]) of every slot of a plan, wide (plan.slot_records) or narrow (plan.desc.slots)"""
    recs = plan.slot_records if getattr(plan, "wide", False) else plan.desc.slots
    return [dict(kind=int(recs[i].kind), state_off=int(recs[i].state_off), p=[float(recs[i].p[j]) for j in range(8)])
            for i in range(plan.n_slots)]


def _step(kind, scheme, T, p, aux, dt, sq, st, w):
    """one sub-model, one sub-step: st = list of the slot's state rows, w = its correlated normal; -> (new rows, pre-floor y | None)"""
    p = [T(v) for v in p]
    aux = [T(v) for v in aux]
    if kind == BS:
        S, sigma, rate = st[0], p[1], p[2]
        if scheme == ANALYTICAL:
            drift = aux[0]                                   # rate * delta_t
            diffusion = w - aux[1]                           # corr_randn - 0.5 * delta_t * sigma**2
            return [S * np.exp(drift + diffusion)], None
        dS = rate * S * dt + sigma * S * sq * w
        return [S + dS], None
    if kind == VASICEK:
        r, logB, sigma, theta, a = st[0], st[1], p[1], p[2], p[3]
        logB_next = logB + r * dt
        if scheme == ANALYTICAL:
            mean = theta + (r - theta) * aux[0]              # exp(-a * delta_t)
            return [mean + w, logB_next], None
        return [r + a * (theta - r) * dt + sigma * sq * w, logB_next], None
    if kind == HW:
        r, logB, sigma, a = st[0], st[1], p[1], p[3]
        logB_next = logB + r * dt
        if scheme == ANALYTICAL:
            return [r * aux[0] + aux[1] + w, logB_next], None
        return [r + (aux[0] - a * r) * dt + sigma * sq * w, logB_next], None
    if kind == CIRPP:
        y, Lam, kappa, theta, sigma = st[0], st[1], p[0], p[1], p[2]
        sqrt_y = np.sqrt(np.maximum(y, T(0.0)))
        y_next = y + kappa * (theta - y) * dt + sigma * sqrt_y * sq * w
        lam = y + aux[0]                                     # lambda_t(time1, y) = y + psi(time1)
        return [np.maximum(y_next, T(FLOOR)), Lam + lam * dt], y_next
    if kind == CIRPP_DET:
        return [np.full_like(st[0], aux[1]), st[1] + aux[0] * dt], None
    raise ValueError(f"model kind {kind} is not a one-factor kind of a wide model")


class Result:
    """paths [n_dates][n_state][n] in the run's dtype; min_y: the smallest CIR++ state before the floor (inf without CIR++ slots)"""


def run(plan, z, dtype=np.float64, start=None) -> Result:
    """z [n_steps][n_z][n] uncorrelated normals (doubles); start [n_state][n] per-path start state or None (the model's own)"""
    T = dtype
    z = np.asarray(z, dtype=np.float64)
    n = z.shape[2] if z.ndim == 3 and z.shape[0] else (np.asarray(start).shape[1] if start is not None else 1)
    slots = slot_records(plan)
    scheme = int(plan.desc.scheme)
    if start is None:
        state = np.tile(np.asarray(plan.init_state, dtype=np.float64)[:, None], (1, n)).astype(T)
    else:
        state = np.asarray(start, dtype=np.float64).astype(T)
    out = np.full((plan.n_dates, plan.n_state, n), np.nan, dtype=T)
    for t in range(plan.n_initial_store):
        out[t] = state
    res = Result()
    res.min_y = np.inf
    for k in range(plan.n_steps):
        dt, sq = T(plan.steps["dt"][k]), T(plan.steps["sqrt_dt"][k])
        L = np.asarray(plan.chol[int(plan.steps["chol_idx"][k])], dtype=np.float64).astype(T)
        w = np.matmul(z[k].astype(T).T, L.T).T                       # corr_randn = z @ L.T, [n_z][n]
        new = state.copy()
        for i, sl in enumerate(slots):
            so, sd = sl["state_off"], STATE_DIM[sl["kind"]]
            rows, y_pre = _step(sl["kind"], scheme, T, sl["p"], plan.aux[k, i], dt, sq, [state[so + c] for c in range(sd)], w[i])
            for c in range(sd):
                new[so + c] = rows[c]
            if y_pre is not None:
                res.min_y = min(res.min_y, float(np.min(y_pre)))
        state = new
        if int(plan.steps["store_idx"][k]) >= 0:
            out[int(plan.steps["store_idx"][k])] = state
    res.paths = out
    return res


def own_rounding(plan, z, start=None) -> tuple[float, Result]:
    """the restatement's own rounding on these inputs: max over stored entries of |float64 run - long double run| relative to the
    largest |entry| of the entry's row (date, state column).  -> (that number, the long-double run)"""
    lo, hi = run(plan, z, np.float64, start), run(plan, z, LD, start)
    return row_relative_gap(lo.paths, hi.paths), hi


def row_relative_gap(got, ref) -> float:
    """max |got - ref| / max_paths |ref| over the rows (date, state column); a row of zeros must be reproduced exactly"""
    ref = np.asarray(ref, dtype=LD)
    err = np.abs(np.asarray(got).astype(LD) - ref).max(axis=2)
    scale = np.abs(ref).max(axis=2)
    assert not ((scale == 0) & (err != 0)).any(), "a row of zeros is not reproduced"
    return float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, LD(1.0)), LD(0.0))))
