"""The dual step maps of the one-factor sub-models with EXPLICIT tangents in plain numpy, float64 or np.longdouble (helper, not a test).

tests/wide_paths_reference.py restates the reference project's time loop for the kinds a wide model may hold; this module carries,
next to every state row, its derivative with respect to NP directions, written out by hand from the same formulas (no dual-number
class, no derived step constants, no fused multiply-adds, not the kernels' evaluation order):

    correlation   w = z @ L.T,                       dw = z @ dL.T   (ANALYTICAL: the factor depends on the parameters; EULER: 0)
    BS     EULER       S' = S + (r S dt + sigma S sqrt(dt) w)
                       dS' = dS + (dr S + r dS) dt + (dsigma S + sigma dS) sqrt(dt) w + sigma S sqrt(dt) dw
           ANALYTICAL  S' = S e,  e = exp(drift + (w - ito));   dS' = dS e + S e (ddrift + dw - dito)
    Vasicek EULER      r' = r + a (theta - r) dt + sigma sqrt(dt) w
                       dr' = dr + (da (theta - r) + a (dtheta - dr)) dt + dsigma sqrt(dt) w + sigma sqrt(dt) dw
           ANALYTICAL  r' = theta + (r - theta) decay + w;  dr' = dtheta + (dr - dtheta) decay + (r - theta) ddecay + dw
           both        logB' = logB + r dt;  dlogB' = dlogB + dr dt
    CIR++  EULER       y' = max(y_next, 1e-12),  y_next = y + kappa (theta - y) dt + sigma sqrt(max(y, 0)) sqrt(dt) w
                       dy_next = dy + (dkappa (theta - y) + kappa (dtheta - dy)) dt + (dsigma s + sigma ds) sqrt(dt) w + sigma s sqrt(dt) dw,
                       s = sqrt(max(y, 0)), ds = dy / (2 s) where y >= 0 and dy != 0, else 0;  dy' = dy_next where y_next >= 1e-12, else 0
                       (torch.clamp passes the gradient on the closed side; its mask discards the infinite root derivative)
                       Lambda' = Lambda + (y + psi) dt;  dLambda' = dLambda + (dy + dpsi) dt
    CIR++ det.         y' = lambda_mkt(t2), Lambda' = Lambda + lambda_mkt(t1) dt, tangents from the aux rows alone

Inputs: the SimPlan tables the kernels read, the tables' derivatives in the layout of mcx_tangent_paths_wide (dslot
[n_slots][8][NP], dinit [n_state][NP], daux [n_steps][n_slots][8][NP], dchol [n_chol][n_z][n_z][NP] or None under EULER) and the
uncorrelated normals.  `own_rounding` runs float64 against np.longdouble: the yardstick of the device tests."""
from __future__ import annotations

import numpy as np

import wide_paths_reference as wr

LD = np.longdouble
BS, VASICEK, CIRPP, CIRPP_DET = wr.BS, wr.VASICEK, wr.CIRPP, wr.CIRPP_DET


class Result:
    """paths [T][D][n], dpaths [NP][T][D][n] in the run's dtype; min_y / min_floor_gap: the smallest CIR++ state before the floor
    and the smallest distance of one to the floor or to zero (inf without stochastic CIR++ slots)"""


def _step(kind, scheme, T, p, dp, aux, daux, dt, sq, st, dst, w, dw, res):
    """one sub-model, one sub-step.  st / dst: the slot's state rows [n] and their tangents [NP][n]; w, dw [NP][n]: its correlated
    normal and that normal's tangent; p, aux scalars with tangents dp, daux [..][NP] -> (new rows, new tangent rows)"""
    col = lambda v: v[:, None]                                   # a [NP] tangent of a scalar against [NP][n] rows
    if kind == BS:
        S, dS = st[0], dst[0]
        if scheme == wr.ANALYTICAL:
            e = np.exp(aux[0] + (w - aux[1]))
            return [S * e], [dS * e + S * e * (col(daux[0]) + dw - col(daux[1]))]
        sigma, rate, dsigma, drate = p[1], p[2], col(dp[1]), col(dp[2])
        dSn = dS + (drate * S + rate * dS) * dt + (dsigma * S + sigma * dS) * sq * w + sigma * S * sq * dw
        return [S + (rate * S * dt + sigma * S * sq * w)], [dSn]
    if kind == VASICEK:
        r, logB, dr, dlogB = st[0], st[1], dst[0], dst[1]
        sigma, theta, a, dsigma, dtheta, da = p[1], p[2], p[3], col(dp[1]), col(dp[2]), col(dp[3])
        logB_n, dlogB_n = logB + r * dt, dlogB + dr * dt
        if scheme == wr.ANALYTICAL:
            decay, ddecay = aux[0], col(daux[0])
            return [theta + (r - theta) * decay + w, logB_n], [dtheta + (dr - dtheta) * decay + (r - theta) * ddecay + dw, dlogB_n]
        rn = r + a * (theta - r) * dt + sigma * sq * w
        drn = dr + (da * (theta - r) + a * (dtheta - dr)) * dt + dsigma * sq * w + sigma * sq * dw
        return [rn, logB_n], [drn, dlogB_n]
    if kind == CIRPP:
        y, Lam, dy, dLam = st[0], st[1], dst[0], dst[1]
        kappa, theta, sigma, dkappa, dtheta, dsigma = p[0], p[1], p[2], col(dp[0]), col(dp[1]), col(dp[2])
        s = np.sqrt(np.maximum(y, T(0.0)))
        with np.errstate(divide="ignore", invalid="ignore"):
            ds = np.where((y >= 0) & (dy != 0), dy / (T(2.0) * s), T(0.0))
        yn = y + kappa * (theta - y) * dt + sigma * s * sq * w
        dyn = dy + (dkappa * (theta - y) + kappa * (dtheta - dy)) * dt + (dsigma * s + sigma * ds) * sq * w + sigma * s * sq * dw
        res.min_y = min(res.min_y, float(np.min(yn)))
        res.min_floor_gap = min(res.min_floor_gap, float(np.min(np.abs(yn - T(wr.FLOOR)))), float(np.min(np.abs(yn))))
        keep = yn >= T(wr.FLOOR)
        return ([np.maximum(yn, T(wr.FLOOR)), Lam + (y + aux[0]) * dt],
                [np.where(keep, dyn, T(0.0)), dLam + (dy + col(daux[0])) * dt])
    if kind == CIRPP_DET:
        n = st[0].shape[0]
        return ([np.full_like(st[0], aux[1]), st[1] + aux[0] * dt],
                [np.repeat(col(daux[1]), n, axis=1), dst[1] + col(daux[0]) * dt])
    raise ValueError(f"model kind {kind} has no dual step")


def run(plan, z, dslot, dinit, daux, dchol=None, dtype=np.float64) -> Result:
    """z [n_steps][n_z][n] uncorrelated normals (doubles); the derivative tables as float64 arrays"""
    T = dtype
    z = np.asarray(z, dtype=np.float64)
    n, NP = z.shape[2], np.asarray(dinit).shape[-1]
    slots = wr.slot_records(plan)
    scheme = int(plan.desc.scheme)
    dslot, dinit, daux = (np.asarray(a, dtype=np.float64).astype(T) for a in (dslot, dinit, daux))
    state = np.tile(np.asarray(plan.init_state, dtype=np.float64)[:, None], (1, n)).astype(T)
    dstate = np.ascontiguousarray(np.repeat(dinit.T[:, :, None], n, axis=2))                  # [NP][D][n]
    out = np.full((plan.n_dates, plan.n_state, n), np.nan, dtype=T)
    dout = np.full((NP, plan.n_dates, plan.n_state, n), np.nan, dtype=T)
    for t in range(plan.n_initial_store):
        out[t], dout[:, t] = state, dstate
    res = Result()
    res.min_y = res.min_floor_gap = np.inf
    for k in range(plan.n_steps):
        dt, sq = T(plan.steps["dt"][k]), T(plan.steps["sqrt_dt"][k])
        f = int(plan.steps["chol_idx"][k])
        L = np.asarray(plan.chol[f], dtype=np.float64).astype(T)
        zk = z[k].astype(T)
        w = np.matmul(zk.T, L.T).T                                                            # [n_z][n]
        dw = np.zeros((NP,) + w.shape, dtype=T)
        if dchol is not None:
            dL = np.asarray(dchol[f], dtype=np.float64).astype(T)                             # [n_z][n_z][NP]
            for q in range(NP):
                dw[q] = np.matmul(zk.T, dL[:, :, q].T).T
        new, dnew = state.copy(), dstate.copy()
        for i, sl in enumerate(slots):
            so, sd = sl["state_off"], wr.STATE_DIM[sl["kind"]]
            rows, drows = _step(sl["kind"], scheme, T, [T(v) for v in sl["p"]], dslot[i], [T(v) for v in plan.aux[k, i]], daux[k, i],
                                dt, sq, [state[so + c] for c in range(sd)], [dstate[:, so + c] for c in range(sd)], w[i], dw[:, i], res)
            for c in range(sd):
                new[so + c], dnew[:, so + c] = rows[c], drows[c]
        state, dstate = new, dnew
        st = int(plan.steps["store_idx"][k])
        if st >= 0:
            out[st], dout[:, st] = state, dstate
    res.paths, res.dpaths = out, dout
    return res


def row_relative_gap(got, ref, scale_from=None) -> float:
    """max |got - ref| / max_paths |ref| over the rows (direction, date, state column); a row of zeros must be reproduced exactly.
    scale_from: the rows' largest entries are taken from this tensor (the same rows on MORE paths) instead of from ref"""
    ref = np.asarray(ref, dtype=LD)
    err = np.abs(np.asarray(got).astype(LD) - ref).max(axis=-1)
    scale = np.abs(ref if scale_from is None else np.asarray(scale_from, dtype=LD)).max(axis=-1)
    assert not ((scale == 0) & (err != 0)).any(), "a row of zeros is not reproduced"
    return float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, LD(1.0)), LD(0.0))))


def own_rounding(plan, z, dslot, dinit, daux, dchol=None) -> tuple[float, Result]:
    """the restatement's own rounding of the TANGENT images on these inputs (float64 run against long-double run, relative to the
    largest entry of a row), floored at n_sub_steps x 2.2e-16 -> (that number, the long-double run)"""
    lo, hi = run(plan, z, dslot, dinit, daux, dchol, np.float64), run(plan, z, dslot, dinit, daux, dchol, LD)
    hi.lo = lo
    return yardstick(lo, hi, z.shape[2], plan.n_steps), hi


def yardstick(lo: Result, hi: Result, n: int, n_steps: int) -> float:
    """own_rounding restricted to the first n paths: a gap measured on n paths is relative to the rows' largest entries AMONG THEM (a
    tangent row can be a small residual of cancelling terms on some paths), and so must its yardstick be"""
    return max(row_relative_gap(lo.dpaths[..., :n], hi.dpaths[..., :n]), n_steps * 2.2e-16)


def active_from_tables(plan, dslot, dinit, daux, dchol=None) -> list:
    """the slots a non-zero table entry reaches, derived here independently of mcx.aad.active_slots"""
    out = []
    for r, sl in enumerate(wr.slot_records(plan)):
        c, dim = sl["state_off"], wr.STATE_DIM[sl["kind"]]
        hit = bool(np.count_nonzero(dslot[r]) + np.count_nonzero(dinit[c:c + dim]) + np.count_nonzero(daux[:, r]))
        if dchol is not None:
            hit = hit or bool(np.count_nonzero(dchol[:, r]))
        if hit:
            out.append(r)
    return out


# ---- the tables' derivatives of a bare simulation, chunked as the forward-mode pass chunks them ---------------------------------------
def derivative_tables(model, plan) -> dict:
    """d (slots, init, aux[, chol]) / d theta_j for every model parameter, [..., P]: the driver's own descriptor tangents
    (mcx.aad.descriptor_tangents, complex step) on a bare simulation — a book without atoms.  Host only"""
    import types
    from mcx import aad
    bare = types.SimpleNamespace(sim_plan=plan, _comp=types.SimpleNamespace(atoms=[], atom_src=[]))
    return aad.descriptor_tangents(bare, model, False, mode="complex")[1]


def chunks(dd, P, NP=4):
    """(parameter indices, zero-padded tables dict(slots, init, aux, chol | None)) per chunk of NP parameters, in parameter order"""
    from mcx import aad
    for c0 in range(0, P, NP):
        sel = list(range(c0, min(c0 + NP, P)))
        d = {k: aad.pad_chunk(v, sel) for k, v in dd.items()}
        d.setdefault("chol", None)
        yield sel, d
