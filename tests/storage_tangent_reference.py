"""Float64 numpy restatement of the storage's sensitivities (test helper; no kernel arithmetic shared) — the checker of
csrc/kt_storage.hip and of `run_with_tangent_book`'s storage branch, next to the reference's autograd fixtures (storage_*_aad.npz).

The derivative is the one of the reference's tape (products/storage.py:219-308): decisions, next states and volume changes carry
no gradient; it flows through cash / numeraire of the chosen action, the interpolated cache at fixed weights, the least-squares
solve and the exposure polynomials.  Three layers:

  * `ComplexStep`: path and atom tangents.  The closed forms of the models (`_slots`, `_step_aux`, `_atom`, `_cholesky_entries`) and
    a numpy restatement of the Schwartz two-factor / Black-Scholes / CIR++ step maps are evaluated at theta_j + i h, h = 1e-30 theta
    scale, on the recorded draws: Im / h is the derivative to rounding, no difference quotient.
  * `StorageTangentRestatement`: the dual recursion in explicit (value, tangents [P]) arrays — roll of the integer grid states,
    dual least squares, walk of the realised state.  `centred=True` solves in the basis of z = (x - mid) / half-range (as the
    kernels' normal equations are posed, through one QR), `centred=False` on the raw monomials through torch.linalg.lstsq and
    torch's reverse mode, as the reference's tape does: their difference is what the raw solve's conditioning costs in a gradient.
  * `restate_case`: a fixture case end to end on the host -> metric gradients (PV, EPE, ENE, PFE, CVA) of every netting set whose
    products are storages or European options on a spot (`restate_european`: payoff and regressed exposure in dual numbers), with
    the symmetric threshold and the margin-period collateral call applied to the netted rows (`unsecured_profile`)."""
import copy
import math

import numpy as np

from storage_reference import _basis, _lerp, _rate


# ---- complex-step paths and atoms ------------------------------------------------------------------------------------------------
def _leaves(model):
    return list(model.models) if hasattr(model, "models") else [model]


def complex_model(model, j, h):
    """a copy of `model` whose closed forms see parameter j (index into get_model_params()) at theta_j + i h"""
    m = copy.deepcopy(model)
    for leaf in _leaves(m):
        n = len(leaf.model_params)
        leaf._complex_step = [complex(float(p.detach()), h if q == j else 0.0) for q, p in enumerate(leaf.model_params)]
        j -= n
    return m


def restate_paths(model, plan, z):
    """paths [T][D][n] (complex when the model's closed forms are) from the draws z [steps][n][n_z] on the sub-step table of `plan`
    (mcx.plan.SimPlan of the real model): EULER for Black-Scholes / CIR++ slots, EULER and ANALYTICAL for the Schwartz two-factor"""
    from mcx import _abi
    slots = model._slots()
    n = z.shape[1]
    init = np.array(model._initial_state(), dtype=np.complex128)
    reg, col = [], 0
    for sp in slots:
        lo = col + (1 if sp.kind == _abi.MODEL_S2F else 0)                        # S2F registers are (x, y) = columns 1, 2
        reg.append([np.full(n, init[lo]), np.full(n, init[lo + 1] if sp.kind != _abi.MODEL_BS else 0.0)])
        col += sp.state_dim
    paths = np.zeros((plan.n_dates, plan.n_state, n), dtype=np.complex128)

    def store(t, aux):
        c = 0
        for s, sp in enumerate(slots):
            if sp.kind == _abi.MODEL_S2F:
                log_f = sp.params[6] if aux is None else aux[s][1]
                paths[t, c], paths[t, c + 1], paths[t, c + 2] = log_f + reg[s][0] + reg[s][1], reg[s][0], reg[s][1]
            else:
                paths[t, c] = reg[s][0]
                if sp.kind != _abi.MODEL_BS:
                    paths[t, c + 1] = reg[s][1]
            c += sp.state_dim

    for t in range(plan.n_initial_store):
        store(t, None)
    analytical = plan.scheme.name == "ANALYTICAL"
    for k in range(plan.n_steps):
        st = plan.steps[k]
        dt, sq, ci = float(st["dt"]), float(st["sqrt_dt"]), int(st["chol_idx"])
        L = np.array(model._cholesky_entries(plan.scheme, plan.chol_dt[ci])) if hasattr(model, "_cholesky_entries") else plan.chol[ci]
        zc = z[k] @ L.T
        aux = model._step_aux(plan.scheme, float(st["t1"]), dt)
        zo = 0
        for s, sp in enumerate(slots):
            p, a = sp.params, aux[s]
            r0, r1 = reg[s]
            if sp.kind == _abi.MODEL_S2F:
                if analytical:
                    reg[s] = [r0 * a[0] + zc[:, zo], r1 + p[3] * dt + zc[:, zo + 1]]
                else:
                    reg[s] = [r0 - p[1] * r0 * dt + p[2] * sq * zc[:, zo], r1 + p[3] * dt + p[4] * sq * zc[:, zo + 1]]
            elif sp.kind == _abi.MODEL_BS:
                assert not analytical
                reg[s] = [r0 + (p[2] * r0 * dt + p[1] * r0 * (sq * zc[:, zo])), r1]
            elif sp.kind == _abi.MODEL_CIRPP:
                assert not analytical
                sy = np.sqrt(np.where(r0.real >= 0.0, r0, 0.0))
                yn = r0 + p[0] * (p[1] - r0) * dt + p[2] * sy * (sq * zc[:, zo])
                reg[s] = [np.where(yn.real >= 1e-12, yn, 1e-12), r1 + (r0 + a[0]) * dt]
            elif sp.kind == _abi.MODEL_CIRPP_DET:
                reg[s] = [np.full(n, a[1], dtype=np.complex128), r1 + a[0] * dt]
            else:
                raise NotImplementedError(f"slot kind {sp.kind}")
            zo += sp.sim_dim
        if st["store_idx"] >= 0:
            store(int(st["store_idx"]), aux)
    return paths


class ComplexStep:
    """values and parameter tangents of the book's atoms on the paths the draws `z` generate: one complex evaluation per parameter"""

    def __init__(self, sc, plan, z):
        from mcx.request_interface.request_types import AtomicRequest, AtomicRequestType
        self._req, self._type = AtomicRequest, AtomicRequestType
        self.sc = sc
        theta = [float(p.detach()) for p in sc.model.get_model_params()]
        self.P = len(theta)
        self.h = [1e-30 * max(abs(t), 1e-2) for t in theta]
        self.models = [complex_model(sc.model, j, self.h[j]) for j in range(self.P)]
        self.paths_c = [restate_paths(m, plan, z) for m in self.models]
        self.paths = restate_paths(sc.model, plan, z).real
        self.dpaths = np.stack([pc.imag / h for pc, h in zip(self.paths_c, self.h)])          # [P][T][D][n]

    def _eval(self, model, paths, atom_id):
        comp = self.sc._comp
        src = comp.atom_src[atom_id]
        n = paths.shape[2]
        if src is None:
            return np.full(n, comp.atoms[atom_id][2], dtype=paths.dtype)
        co = model._atom(*src)
        x = paths[comp.atoms[atom_id][0], co.col] if co.col is not None else np.zeros(n, dtype=paths.dtype)
        v = co.a + co.d * x
        return v + co.b * np.exp(co.c0 + co.c1 * x) if co.b != 0.0 else v

    def value(self, atom_id):
        """-> (value [n], tangents [P][n])"""
        v = self._eval(self.sc.model, self.paths, atom_id)
        dv = np.stack([np.imag(self._eval(m, pc, atom_id)) / h for m, pc, h in zip(self.models, self.paths_c, self.h)])
        return np.real(v), dv

    def spot(self, asset, t):
        return self.value(self.sc._comp.atom(self._req(self._type.SPOT), asset, float(t)))

    def numeraire(self, t):
        return self.value(self.sc._comp.atom(self._req(self._type.NUMERAIRE, float(t)), "numeraire", float(t)))


# ---- dual least squares ------------------------------------------------------------------------------------------------------------
def lstsq_dual(A, dA, Y, dY):
    """c = argmin |A c - Y| and its tangents at full rank: dc = A^+ (dY - dA c) + (A^T A)^-1 dA^T (Y - A c), through one QR of A.
    A [n][K], dA [P][n][K], Y [n][S], dY [P][n][S] -> c [S][K], dc [P][S][K]"""
    Q, R = np.linalg.qr(A)
    c = np.linalg.solve(R, Q.T @ Y)
    res = Y - A @ c
    dc = np.stack([np.linalg.solve(R, Q.T @ (dY[q] - dA[q] @ c)) + np.linalg.solve(R, np.linalg.solve(R.T, dA[q].T @ res))
                   for q in range(len(dA))])
    return c.T, np.transpose(dc, (0, 2, 1))


def lstsq_dual_tape(A, dA, Y, dY):
    """the same derivative obtained as the reference obtains it: torch.linalg.lstsq on the raw system, differentiated by torch's
    reverse mode (its backward goes through the pseudo-inverse, so the conditioning of the raw monomial basis enters squared and is
    multiplied by the residual).  One scalar theta per tangent direction: A + theta dA, Y + theta dY."""
    import torch
    K, S = A.shape[1], Y.shape[1]
    At, Yt = torch.from_numpy(np.ascontiguousarray(A)), torch.from_numpy(np.ascontiguousarray(Y))
    c = torch.linalg.lstsq(At, Yt).solution.numpy()
    dc = np.zeros((len(dA), S, K))
    eye = torch.eye(K * S, dtype=torch.float64).reshape(K * S, K, S)
    for q in range(len(dA)):
        th = torch.zeros((), dtype=torch.float64, requires_grad=True)
        sol = torch.linalg.lstsq(At + th * torch.from_numpy(np.ascontiguousarray(dA[q])), Yt + th * torch.from_numpy(np.ascontiguousarray(dY[q]))).solution
        g, = torch.autograd.grad(sol, th, grad_outputs=eye, is_grads_batched=True)
        dc[q] = g.numpy().reshape(K, S).T
    return c.T, dc


def solve_dual(x, dx, Y, dY, K, centred):
    """the regression of Y [n][S] on the monomials of x with tangents -> coefficients of x^k [S][K], [P][S][K]"""
    P, S = len(dx), Y.shape[1]
    if not x.max() > x.min():
        # every path shares x = x0 (the calibration date): the minimum-norm solution c = v ybar / (v.v), v = [1, x0, .., x0^(K-1)]
        x0, dx0 = x[0], dx[:, 0]
        v = np.array([x0 ** k for k in range(K)])
        dv = np.array([k * x0 ** (k - 1) if k else 0.0 for k in range(K)])
        vv = float(v @ v)
        ybar, dybar = Y.mean(axis=0), dY.mean(axis=1)
        c = ybar[:, None] * v[None, :] / vv
        dc = np.zeros((P, S, K))
        for q in range(P):
            dvq = dv * dx0[q]
            dc[q] = (dybar[q][:, None] * v[None, :] + ybar[:, None] * dvq[None, :]) / vv - ybar[:, None] * v[None, :] * (2.0 * float(v @ dvq) / vv ** 2)
        return c, dc
    dbasis = lambda u, du: np.stack([np.stack([k * u ** (k - 1) * du[q] if k else np.zeros_like(u) for k in range(K)], axis=1) for q in range(P)])
    if not centred:
        return lstsq_dual_tape(_basis(x, K), dbasis(x, dx), Y, dY)
    mid, half = 0.5 * (x.min() + x.max()), 0.5 * (x.max() - x.min())          # constants: the range is not differentiated
    z, dz = (x - mid) / half, dx / half
    b, db = lstsq_dual(_basis(z, K), dbasis(z, dz), Y, dY)
    T = np.zeros((K, K))
    for k in range(K):
        for j in range(k + 1):
            T[j, k] = math.comb(k, j) * (-mid) ** (k - j) / half ** k
    return b @ T.T, db @ T.T


# ---- the storage in dual numbers -----------------------------------------------------------------------------------------------------
def _lerp_fixed(dvalues, state, S):
    """tangent arrays [P][n][S] interpolated at PRIMAL states [n][B] with their primal weights"""
    return np.stack([_lerp(dv, state) for dv in dvalues])


class StorageTangentRestatement:
    def __init__(self, product, K, float32_quirk=True, centred=True, float32_tangent=False):
        """float32_tangent: also round the step buffer's TANGENT to float32.  The reference's tape carries its adjoints through the
        float32 step buffer (controller.py:330-351), so its gradients hold float32 rounding that the regression then amplifies;
        this switch reproduces the size of that effect (not its digits: adjoints are rounded there, tangents here)."""
        self.p, self.K, self.f32, self.centred, self.f32_tangent = product, K, float32_quirk, centred, float32_tangent
        self.S = product.get_num_states()
        self.dates = [float(t) for t in product.product_timeline]
        self.next_dates = [float(t) for t in product.next_action_dates]

    def step(self, j, state, spot, dspot, num, dnum, coeffs):
        """one action date for states [n][B] under the decisions `coeffs` [S][K] imply on the PRIMAL values
        -> next state [n][B], cash / numeraire [n][B] and its tangents [P][n][B]"""
        p, cfg, S = self.p, self.p.storage_config, self.S
        t, nxt = self.dates[j], self.next_dates[j]
        w, nw = cfg.get_volume_constraint(t), cfg.get_volume_constraint(nxt)
        step = 0.0 if np.isclose(w.vmin, w.vmax, rtol=0.0, atol=1e-12) else (w.vmax - w.vmin) / (S - 1.0)
        scale = 0.0 if np.isclose(nw.vmin, nw.vmax, rtol=0.0, atol=1e-12) else (S - 1.0) / (nw.vmax - nw.vmin)
        period = max(nxt - t, 0.0)
        v = w.vmin + state * step
        nv = np.stack([np.minimum(v + _rate(cfg.get_injection_flexibility_slice(t), v) * period, nw.vmax),
                       np.clip(v, nw.vmin, nw.vmax),
                       np.maximum(v - _rate(cfg.get_withdrawal_flexibility_slice(t), v) * period, nw.vmin)], axis=2)
        ns = np.zeros_like(nv) if scale == 0.0 else (nv - nw.vmin) * scale
        dv = nv - v[:, :, None]
        buy, sell = (spot + cfg.get_variable_injection_cost(t))[:, None], (spot - cfg.get_variable_withdrawal_cost(t))[:, None]
        price = np.stack([np.broadcast_to(buy, v.shape), np.where(dv[:, :, 1] >= 0.0, buy, sell), np.broadcast_to(sell, v.shape)], axis=2)
        cash = -dv * price
        value = cash.copy()
        if not nxt >= p.end_date - 1e-12:
            grid = _basis(spot, self.K) @ coeffs.T
            for a in range(3):
                value[:, :, a] += _lerp(grid, ns[:, :, a])
        best = np.argmax(value, axis=2)[:, :, None]                                    # the first maximum; no gradient through it
        pick = lambda m: np.take_along_axis(m, best, axis=2)[:, :, 0]
        cf = pick(cash) / num[:, None]
        # d(cash / num) = (-dv dspot - (cash / num) dnum) / num: the price's tangent is the spot's, dv has none
        dcf = (-pick(dv)[None] * dspot[:, :, None] - cf[None] * dnum[:, :, None]) / num[None, :, None]
        return pick(ns), cf, dcf

    def backward(self, exposure_times, spot_at, numeraire_at, decide):
        """the induction over the regression timeline with tangents.  decide [dates][S][K]: the coefficients decisions are taken
        from (the base run's).  -> {t_reg: dict(coeffs [S][K], dcoeffs [P][S][K])}"""
        pt = np.array(self.dates)
        reg_tl = sorted(set(self.dates) | {float(t) for t in exposure_times})
        x0, dx0 = spot_at(reg_tl[0])
        n, P = len(x0), len(dx0)
        last = len(pt)
        cache, dcache = {last: np.zeros((n, self.S))}, {last: np.zeros((P, n, self.S))}
        out = {}
        for t_reg in reversed(reg_tl):
            idx = int(np.searchsorted(pt, t_reg))
            if idx >= len(pt):
                continue
            t_next = idx + 1 if pt[idx] == t_reg else idx
            if t_next < last:
                state = np.tile(np.arange(self.S, dtype=np.float64), (n, 1))
                step_value = np.zeros((n, self.S), dtype=np.float32 if self.f32 else np.float64)
                dstep = np.zeros((P, n, self.S))
                for j in range(t_next, last):
                    (sp, dsp), (nu, dnu) = spot_at(pt[j]), numeraire_at(pt[j])
                    state, cf, dcf = self.step(j, state, sp, dsp, nu, dnu, decide[j])
                    step_value += cf.astype(step_value.dtype)                     # the float32 step buffer holds the VALUE only
                    dstep += dcf.astype(np.float32).astype(np.float64) if self.f32_tangent else dcf
                cache[t_next] = step_value.astype(np.float64) + _lerp(cache[last], state)
                dcache[t_next] = dstep + _lerp_fixed(dcache[last], state, self.S)
                last = t_next
            (x, dx), (nu, dnu) = spot_at(t_reg), numeraire_at(t_reg)
            total, dtotal = cache[t_next], dcache[t_next]
            Y = nu[:, None] * total
            dY = dnu[:, :, None] * total[None] + nu[None, :, None] * dtotal
            c, dc = solve_dual(x, dx, Y, dY, self.K, self.centred)
            out[t_reg] = dict(coeffs=c, dcoeffs=dc, W=total.T.copy(), dW=np.transpose(dtotal, (0, 2, 1)).copy())
        return out

    def forward(self, exposure_times, want_cfs, spot_at, numeraire_at, decide, expo_coeffs, expo_dcoeffs):
        """the walk of the realised state -> cashflows [n] + tangents [P][n], exposures [E][n] + tangents [P][E][n]"""
        pt, K = self.dates, self.K
        x0, dx0 = spot_at(pt[0])
        n, P = len(x0), len(dx0)
        state, cfs, dcfs = np.zeros((n, 1)), np.zeros(n), np.zeros((P, n))
        j, expo, dexpo = 0, [], []

        def act(j):
            nonlocal state, cfs, dcfs
            (sp, dsp), (nu, dnu) = spot_at(pt[j]), numeraire_at(pt[j])
            state, cf, dcf = self.step(j, state, sp, dsp, nu, dnu, decide[j])
            cfs, dcfs = cfs + cf[:, 0], dcfs + dcf[:, :, 0]

        for i, t in enumerate(float(t) for t in exposure_times):
            while j < len(pt) and pt[j] <= t:
                act(j)
                j += 1
            (x, dx), (nu, dnu) = spot_at(t), numeraire_at(t)
            B = _basis(x, K)
            dBdx = np.stack([k * x ** (k - 1) if k else np.zeros_like(x) for k in range(K)], axis=1)
            g = _lerp(B @ expo_coeffs[i].T, state)[:, 0]
            gx = _lerp(dBdx @ expo_coeffs[i].T, state)[:, 0]                       # d grid / dx at the fixed state
            e = g / nu
            de = np.stack([(_lerp(B @ expo_dcoeffs[q][i].T, state)[:, 0] + gx * dx[q] - e * dnu[q]) / nu for q in range(P)])
            expo.append(e)
            dexpo.append(de)
        if want_cfs or len(exposure_times) == 0:
            while j < len(pt):
                act(j)
                j += 1
        E = len(expo)
        return cfs, dcfs, (np.stack(expo) if E else np.zeros((0, n))), (np.stack(dexpo, axis=1) if E else np.zeros((P, 0, n)))


# ---- a fixture case end to end -------------------------------------------------------------------------------------------------------
def restate_storage(sc, p_i, pre, main, decide, centred=True, float32_quirk=True, float32_tangent=False):
    """one storage of a compiled controller on the atoms of `pre` / `main` (ComplexStep) -> dict of arrays"""
    p, K = sc.products[p_i], sc.regression_function.get_degree()
    asset = p.asset_ids[0]
    rs = StorageTangentRestatement(p, K, float32_quirk, centred, float32_tangent)
    expo_times = [float(t) for t in sc.exposure_timeline] if sc.risk_metrics.requires_exposure_profiles() else []
    back = rs.backward(expo_times, lambda t: pre.spot(asset, t), pre.numeraire, decide)
    P = pre.P
    zero, dzero = np.zeros((rs.S, K)), np.zeros((P, rs.S, K))
    expo_c = np.stack([back[t]["coeffs"] if t in back else zero for t in expo_times]) if expo_times else np.zeros((0, rs.S, K))
    expo_dc = np.stack([back[t]["dcoeffs"] if t in back else dzero for t in expo_times], axis=1) if expo_times else np.zeros((P, 0, rs.S, K))
    cfs, dcfs, expo, dexpo = rs.forward(expo_times, True, lambda t: main.spot(asset, t), main.numeraire, decide, expo_c, expo_dc)
    return dict(back=back, expo_coeffs=expo_c, expo_dcoeffs=expo_dc, cfs=cfs, dcfs=dcfs, expo=expo, dexpo=dexpo, rs=rs)


def restate_european(sc, p_i, pre, main, centred=True):
    """a European option on the spot of one asset (one state, no decision): the payoff over the numeraire and its tangents, and the
    exposure rows the regression of the discounted payoff on that spot gives — dates at or after the exercise date own no cashflow,
    so their coefficients are zero (controller `_regression_schedule`: cashflows strictly after the regression date)"""
    p, K = sc.products[p_i], sc.regression_function.get_degree()
    assert type(p).__name__ == "EuropeanOption" and type(p.underlying).__name__ == "Equity", "restated: options on a spot only"
    asset, T_ex, strike, sign = p.asset_ids[0], float(p.exercise_date[0]), float(p.strike[0]), p._sign()
    P = pre.P

    def payoff(atoms):
        (sp, dsp), (nu, dnu) = atoms.spot(asset, T_ex), atoms.numeraire(T_ex)
        itm = sign * (sp - strike) > 0.0
        cf = np.where(itm, sign * (sp - strike), 0.0) / nu
        return cf, (np.where(itm, sign, 0.0)[None] * dsp - cf[None] * dnu) / nu[None]

    cf_pre, dcf_pre = payoff(pre)
    cfs, dcfs = payoff(main)
    expo_times = [float(t) for t in sc.exposure_timeline] if sc.risk_metrics.requires_exposure_profiles() else []
    n = len(cfs)
    expo_c, expo_dc, expo, dexpo = np.zeros((len(expo_times), 1, K)), np.zeros((P, len(expo_times), 1, K)), [], []
    for i, t in enumerate(expo_times):
        if t < T_ex:
            (x, dx), (nu, dnu) = pre.spot(asset, t), pre.numeraire(t)
            Y, dY = (nu * cf_pre)[:, None], (dnu * cf_pre[None] + nu[None] * dcf_pre)[:, :, None]
            expo_c[i], expo_dc[:, i] = solve_dual(x, dx, Y, dY, K, centred)
        (x, dx), (nu, dnu) = main.spot(asset, t), main.numeraire(t)
        B = _basis(x, K)
        dBdx = np.stack([k * x ** (k - 1) if k else np.zeros_like(x) for k in range(K)], axis=1)
        e = (B @ expo_c[i, 0]) / nu
        gx = dBdx @ expo_c[i, 0]
        expo.append(e)
        dexpo.append(np.stack([(B @ expo_dc[q, i, 0] + gx * dx[q] - e * dnu[q]) / nu for q in range(P)]))
    E = len(expo)
    return dict(expo_coeffs=expo_c, expo_dcoeffs=expo_dc, cfs=cfs, dcfs=dcfs, expo=np.stack(expo) if E else np.zeros((0, n)),
                dexpo=np.stack(dexpo, axis=1) if E else np.zeros((P, 0, n)))


def unsecured_profile(sc, ns_i, expo, dexpo):
    """the rows the exposure metrics see (products/netting_set.py): the netted rows of the metric dates, minus the collateral call
    — the thresholded netted exposure one margin period earlier, zero where that date precedes the grid — for a collateralised set;
    the thresholded rows otherwise.  The threshold map is x -> x -+ h outside [-h, h] and 0 inside: slope 1 or 0.
    -> u [R][n], du [P][R][n]"""
    ns = sc.netting_sets[ns_i]
    rows = sc.metric_exposure_indices.numpy().astype(int)
    h = float(ns.threshold)

    def thr(e, de):
        if h == 0.0:
            return e, de
        out = np.abs(e) > h
        return np.where(out, e - np.sign(e) * h, 0.0), out[None] * de

    u, du = expo[rows].copy(), dexpo[:, rows].copy()
    if not ns.is_collateralized():
        return thr(u, du)
    delayed = sc.netting_set_delayed_exposure_indices[ns_i].numpy().astype(int)
    for m, d in enumerate(delayed):
        if d >= 0:
            c, dc = thr(expo[d], dexpo[:, d])
            u[m] -= c
            du[:, m] -= dc
    return u, du


def metric_gradients(sc, ns_i, cfs, dcfs, expo, dexpo, main):
    """gradients [evaluations][P] of the native metrics of a netting set from per-path netted values and tangents: PV mean; on the
    unsecured rows u (`unsecured_profile`) EPE / ENE the mean over the paths on that side (torch.relu: zero gradient at 0); PFE the
    tangent of the path that realises the order statistic; CVA sum_m relu(u_m) S(0, t_m) (1 - S(t_m, t_m+1)) (1 - R)"""
    from mcx.metrics.metric import MetricType
    ns = sc.netting_sets[ns_i]
    P, n = dcfs.shape
    if sc.risk_metrics.requires_exposure_profiles():
        u_all, du_all = unsecured_profile(sc, ns_i, expo, dexpo)
    else:
        u_all, du_all = np.zeros((0, n)), np.zeros((P, 0, n))
    rows = np.arange(len(u_all))
    expo, dexpo = u_all, du_all
    out = {}
    for m_i, m in enumerate(sc.risk_metrics.metrics):
        if m.metric_type == MetricType.PV:
            g = dcfs.mean(axis=1)[None, :]
        elif m.metric_type in (MetricType.EPE, MetricType.ENE):
            side = (expo[rows] > 0.0) if m.metric_type == MetricType.EPE else (expo[rows] < 0.0)
            g = np.stack([(side * dexpo[q][rows]).mean(axis=1) for q in range(P)], axis=1)
        elif m.metric_type == MetricType.PFE:
            k = m.q_index(n)
            g = np.zeros((len(rows), P))
            for e_i, r in enumerate(rows):
                target = np.sort(expo[r])[k]
                first = int(np.flatnonzero(expo[r] == target)[0])
                g[e_i] = dexpo[:, r, first]
        elif m.metric_type == MetricType.CVA:
            if ns.counterparty_id is not None and m.counterparty_id != ns.counterparty_id:
                g = np.zeros((1, P))
            else:
                surv, cond = sc._cva_atoms[m_i]
                acc = np.zeros((P, n))
                for k in range(len(rows) - 1):
                    u, du = expo[rows[k]], dexpo[:, rows[k]]
                    (s, ds), (c, dc) = main.value(surv[k]), main.value(cond[k])
                    pos = u > 0.0
                    acc += pos * (du * s * (1.0 - c) + u * ds * (1.0 - c) - u * s * dc)
                g = (acc.mean(axis=1) * (1.0 - m.recovery_rate))[None, :]
        else:
            continue
        out[f"{ns_i}_{m_i}"] = g
    return out


def restate_case(name, centred=True, float32_tangent=False):
    """a case of tests/storage_cases.py on the host, from the base fixture's draws -> dict(grads {"<ns>_<metric>": [evals][P]},
    per storage the arrays of restate_storage).  Decisions come from the base fixture's product coefficients."""
    import storage_cases
    from mcx.common.enums import SimulationScheme
    from mcx.plan import SimPlan
    from test_storage_reference import compiled_controller, storages_of
    sc, g = compiled_controller(name)
    _build, _n_pre, _n_main, steps, scheme, _degree = storage_cases.CASES[name]
    plan = SimPlan(sc.model, sc.simulation_timeline.numpy(), getattr(SimulationScheme, scheme), steps)
    pre, main = ComplexStep(sc, plan, g["z_pre"]), ComplexStep(sc, plan, g["z_main"])
    out = dict(grads={}, storages={}, europeans={}, sc=sc, pre=pre, main=main)
    for p_i in storages_of(sc):
        out["storages"][p_i] = restate_storage(sc, p_i, pre, main, g[f"prod_coeffs_{p_i}"], centred, sc.reference_float32_cf_cache, float32_tangent)
    for ns_i, ns in enumerate(sc.netting_sets):
        mine = [i for i in range(len(sc.products)) if sc.product_to_netting_set_idx[i] == ns_i]
        if not all(i in out["storages"] or type(sc.products[i]).__name__ == "EuropeanOption" for i in mine):
            continue
        for i in mine:
            if i not in out["storages"] and i not in out["europeans"]:
                out["europeans"][i] = restate_european(sc, i, pre, main, centred)
        r = [out["storages"][i] if i in out["storages"] else out["europeans"][i] for i in mine]
        out["grads"].update(metric_gradients(sc, ns_i, sum(x["cfs"] for x in r), sum(x["dcfs"] for x in r), sum(x["expo"] for x in r),
                                             sum(x["dexpo"] for x in r), main))
    return out
