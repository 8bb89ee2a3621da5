"""The twelve step maps of the path kernels in long double, with a derived first-order rounding-error bound per output entry.

Plain numpy on np.longdouble; no torch, nothing of the library under test.  `advance` takes a block of paths from one stored date
to the next through its sub-steps.  Its inputs are exactly the doubles a kernel gets: the SimPlan tables (steps, aux, chol, slot
parameters, flags), the stored state, the uncorrelated normals and the uniform of every sub-step.  It applies z @ L.T and then the
per-slot maps, written from the formulas of the reference project (models/<model>.py, cited per map) — not from the evaluation
order of the kernels.  The derived Euler step constants of mcx_sim_create (r dt, sigma sqrt(dt), a theta dt, -(a dt) ...) are
modelled as rounded intermediates like every other operation.

The bound.  Every rounded operation (product, sum, quotient, root, log, exp; the argument of a log or exp is itself the result of
one) goes through `Ops.r`, which can multiply ONE chosen operation by (1 + delta).  With d = 2^-30

    sens = sum_k max(|out(delta_k = +d) - out|, |out(delta_k = -d) - out|) / d

and an implementation whose operations have relative error <= u each lands within u * sens of the long-double value, to first
order.  Both signs are taken so that the continuous kinks (max, min, clamp, the fuzzy degree of truth) are bounded from either
side.  u = U_KERNEL = 2^-50 covers what the kernels document (0.5 ulp fma / add / multiply, <= 1 ulp mcx_rcp / mcx_sqrt / mcx_log /
mcx_exp, 1-2 ulp mcx_sqrt_g(p), ~3 ulp for a reciprocal recovered from a grouped v_rcp_f64); u = U_IEEE = 2^-52 is for the IEEE
oracle.  Draws are exact inputs.

Besides value and sens, `advance` returns per sub-step the two hard-indicator margins of the QE step (u - p, psi - 1.5) and
psi + eps, each with its own sens, and a NaN mask where the reference takes the root of a negative 2 / psi under smoothing.

`check_paths` is the harness of tests/test_step_reference.py (oracle backend, CPU) and tests/test_step_kernels.py (every GPU
route): every transition between stored dates starts from the checked implementation's OWN stored state, so errors do not
accumulate and any kernel that writes paths can be checked.

`mut=` replaces the reference by a subtly wrong map (MUTATIONS): the harness must then fail — the proof that the committed inputs
reach the floor, the cap, both QE branches, a non-trivial factor and a non-uniform grid."""
from __future__ import annotations

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "step_reference needs an extended-precision long double"

U_KERNEL = 2.0 ** -50
U_IEEE = 2.0 ** -52
D_FD = LD(2.0) ** -30

SCHEME_EULER, SCHEME_ANALYTICAL, SCHEME_QE = 0, 2, 3
BS, HESTON, VASICEK, CIRPP, CIRPP_DET, HW, S2F = 1, 2, 3, 4, 5, 6, 7
FLAG_SMOOTHING = 1
STATE_DIM = {BS: 1, HESTON: 2, VASICEK: 2, CIRPP: 2, CIRPP_DET: 2, HW: 2, S2F: 3}
SIM_DIM = {BS: 1, HESTON: 2, VASICEK: 1, CIRPP: 1, CIRPP_DET: 1, HW: 1, S2F: 2}
_KIND_NAME = {BS: "BS", HESTON: "HESTON", VASICEK: "VAS", CIRPP: "CIR", CIRPP_DET: "CIRDET", HW: "HW", S2F: "S2F"}
_SCHEME_NAME = {SCHEME_EULER: "E", SCHEME_ANALYTICAL: "A", SCHEME_QE: "QE"}

MUTATIONS = ("psi_eps", "omu_floor", "p_cap", "k1_k2", "right_endpoint", "cir_floor", "sqrt_abs", "chol_transposed", "aux_next",
             "column_1e-13")

EPS = LD(1e-12)
P_CAP = LD(1.0 - 1e-6)


class Tables:
    """the doubles of a SimPlan that the kernels read"""

    def __init__(self, plan):
        d = plan.desc
        self.scheme, self.n_state, self.n_z, self.n_steps = int(d.scheme), int(d.n_state), int(d.n_z), int(d.n_steps)
        self.dt = np.array(plan.steps["dt"], dtype=np.float64)
        self.sqrt_dt = np.array(plan.steps["sqrt_dt"], dtype=np.float64)
        self.chol_idx = np.array(plan.steps["chol_idx"], dtype=np.int64)
        self.store_idx = np.array(plan.steps["store_idx"], dtype=np.int64)
        self.aux = np.array(plan.aux, dtype=np.float64)             # [n_steps][n_slots][8]
        self.chol = np.array(plan.chol, dtype=np.float64)           # [n_chol][n_z][n_z]
        self.n_initial_store = int(d.n_initial_store)
        self.init_state = np.array(plan.init_state, dtype=np.float64)
        self.slots = []
        for i in range(int(d.n_slots)):
            s = d.slots[i]
            self.slots.append(dict(kind=int(s.kind), state_off=int(s.state_off), z_off=int(s.z_off), flags=int(s.flags) | int(d.flags),
                                   p=np.array([float(s.p[j]) for j in range(8)])))

    def map_name(self, slot: int) -> str:
        return _KIND_NAME[self.slots[slot]["kind"]] + "_" + _SCHEME_NAME[self.scheme]

    def transitions(self):
        """[(date_from, date_to, first sub-step, number of sub-steps)] between consecutive stored dates; date_from = -1: the
        model's own start state (a timeline that does not begin at the calibration date stores no start state)"""
        out, k0, prev = [], 0, self.n_initial_store - 1
        for k in range(self.n_steps):
            if self.store_idx[k] >= 0:
                out.append((prev, int(self.store_idx[k]), k0, k - k0 + 1))
                prev, k0 = int(self.store_idx[k]), k + 1
        return out


class Ops:
    """hooked arithmetic: operation number `target` is multiplied by (1 + delta)"""

    def __init__(self, target=-1, delta=0.0, start=0):
        self.n, self.target, self.f, self.kinds = start, target, LD(1.0) + LD(delta), {}

    def r(self, x, kind="op"):
        k = self.n
        self.n += 1
        self.kinds[k] = kind
        return x * self.f if k == self.target else x

    def add(self, a, b): return self.r(a + b, "add")
    def sub(self, a, b): return self.r(a - b, "sub")
    def mul(self, a, b): return self.r(a * b, "mul")
    def div(self, a, b): return self.r(a / b, "div")
    def sqrt(self, a): return self.r(np.sqrt(a), "sqrt")
    def log(self, a): return self.r(np.log(a), "log")
    def exp(self, a): return self.r(np.exp(a), "exp")


def _dot(x, fuzzy, eps, o):
    """maths/maths.py:3-9 compute_degree_of_truth"""
    if not fuzzy:
        return np.where(x > 0, LD(1.0), LD(0.0))
    v = o.div(o.add(x, LD(eps)), LD(2.0 * eps))
    return np.minimum(np.maximum(v, LD(0.0)), LD(1.0))            # (NaN stays NaN)


def _bs(o, tb, k, sl, st, zc, u, mut, mon):
    S, p, dt, sq = st[0], sl["p"], LD(tb.dt[k]), LD(tb.sqrt_dt[k])
    aux = tb.aux[_aux_row(tb, k, mut), sl["i"]]
    if tb.scheme == SCHEME_ANALYTICAL:                             # black_scholes.py:61-67
        diffusion = o.sub(zc[0], LD(aux[1]))
        return [o.mul(S, o.exp(o.add(LD(aux[0]), diffusion)))]
    c0, c2 = o.mul(LD(p[2]), dt), o.mul(LD(p[1]), sq)              # black_scholes.py:79-85 with the derived step constants
    return [o.add(S, o.mul(S, o.add(o.mul(c2, zc[0]), c0)))]


def _aux_row(tb, k, mut):
    return min(k + 1, tb.n_steps - 1) if mut == "aux_next" else k


def _vasicek(o, tb, k, sl, st, zc, u, mut, mon):
    r, logB, p, dt, sq = st[0], st[1], sl["p"], LD(tb.dt[k]), LD(tb.sqrt_dt[k])
    aux = tb.aux[_aux_row(tb, k, mut), sl["i"]]
    sigma, theta, a = LD(p[1]), LD(p[2]), LD(p[3])
    if tb.scheme == SCHEME_ANALYTICAL:                             # vasicek.py:82-84
        rn = o.add(o.add(theta, o.mul(o.sub(r, theta), LD(aux[0]))), zc[0])
    else:                                                          # vasicek.py:108-110, constants of mcx_sim_create
        c0, c1, c2 = o.mul(o.mul(a, theta), dt), -o.mul(a, dt), o.mul(sigma, sq)
        rn = o.add(o.add(o.add(r, o.mul(c1, r)), o.mul(c2, zc[0])), c0)
    integrand = rn if mut == "right_endpoint" else r               # vasicek.py:80 / :107: left endpoint
    return [rn, o.add(logB, o.mul(integrand, dt))]


def _hw(o, tb, k, sl, st, zc, u, mut, mon):
    r, logB, p, dt, sq = st[0], st[1], sl["p"], LD(tb.dt[k]), LD(tb.sqrt_dt[k])
    aux = tb.aux[_aux_row(tb, k, mut), sl["i"]]
    sigma, a = LD(p[1]), LD(p[3])
    if tb.scheme == SCHEME_ANALYTICAL:                             # hull_white.py:76-83
        rn = o.add(o.add(o.mul(r, LD(aux[0])), LD(aux[1])), zc[0])
    else:                                                          # hull_white.py:104-108
        drift = o.mul(o.sub(LD(aux[0]), o.mul(a, r)), dt)
        rn = o.add(o.add(r, drift), o.mul(o.mul(sigma, sq), zc[0]))
    integrand = rn if mut == "right_endpoint" else r
    return [rn, o.add(logB, o.mul(integrand, dt))]


def _cirpp(o, tb, k, sl, st, zc, u, mut, mon):
    y, L, p, dt, sq = st[0], st[1], sl["p"], LD(tb.dt[k]), LD(tb.sqrt_dt[k])       # cirpp.py:188-198
    aux = tb.aux[_aux_row(tb, k, mut), sl["i"]]
    kappa, theta, sigma = LD(p[0]), LD(p[1]), LD(p[2])
    sy = o.sqrt(np.abs(y) if mut == "sqrt_abs" else np.maximum(y, LD(0.0)))
    c0, c1, c2 = o.mul(o.mul(kappa, theta), dt), -o.mul(kappa, dt), o.mul(sigma, sq)
    yn = o.add(o.add(o.add(y, o.mul(c1, y)), o.mul(o.mul(c2, sy), zc[0])), c0)
    yn = np.maximum(yn, LD(0.0) if mut == "cir_floor" else EPS)
    mon["floored"] = yn == EPS
    lam = o.add(yn if mut == "right_endpoint" else y, LD(aux[0]))                  # lambda_t(time1, y): cirpp.py:196, 240-244
    return [yn, o.add(L, o.mul(lam, dt))]


def _cirpp_det(o, tb, k, sl, st, zc, u, mut, mon):                                 # cirpp.py:155-172
    aux = tb.aux[_aux_row(tb, k, mut), sl["i"]]
    return [np.full_like(st[0], LD(aux[1])), o.add(st[1], o.mul(LD(aux[0]), LD(tb.dt[k])))]


def _s2f(o, tb, k, sl, st, zc, u, mut, mon):                                       # schwartz_two_factor.py:147-196
    x, y, p, dt, sq = st[1], st[2], sl["p"], LD(tb.dt[k]), LD(tb.sqrt_dt[k])
    aux = tb.aux[_aux_row(tb, k, mut), sl["i"]]
    kappa, sigma_s, mu, sigma_l = LD(p[1]), LD(p[2]), LD(p[3]), LD(p[4])
    if tb.scheme == SCHEME_ANALYTICAL:
        xn = o.add(o.mul(x, LD(aux[0])), zc[0])
        yn = o.add(o.add(y, o.mul(mu, dt)), zc[1])
    else:
        xn = o.add(o.sub(x, o.mul(o.mul(kappa, x), dt)), o.mul(o.mul(sigma_s, sq), zc[0]))
        yn = o.add(o.add(y, o.mul(mu, dt)), o.mul(o.mul(sigma_l, sq), zc[1]))
    return [o.add(o.add(LD(aux[1]), xn), yn), xn, yn]


def qe_terms(tb, k, v, slot=0):
    """m, psi, p, b of the QE step (heston.py:185-220) in long double for variance v: what the edge states are solved from"""
    o, sl = Ops(), dict(tb.slots[slot], i=slot)
    mon = {}
    z = np.zeros_like(np.asarray(v, dtype=LD))
    _heston(o, tb, k, sl, [z, np.asarray(v, dtype=LD)], [z, z], z + LD(0.5), None, mon)
    return mon


def _heston(o, tb, k, sl, st, zc, u, mut, mon, flip=None):
    logS, v, p, dt, sq = st[0], st[1], sl["p"], LD(tb.dt[k]), LD(tb.sqrt_dt[k])
    sigma, rate, kappa, theta = LD(p[1]), LD(p[2]), LD(p[4]), LD(p[5])
    if tb.scheme == SCHEME_EULER:                                                  # heston.py:109-121
        sv = o.sqrt(np.abs(v) if mut == "sqrt_abs" else np.maximum(v, LD(0.0)))
        drift = o.mul(o.sub(rate, o.mul(LD(0.5), v)), dt)
        logSn = o.add(o.add(logS, drift), o.mul(o.mul(sv, sq), zc[0]))
        vdrift = o.mul(o.mul(kappa, o.sub(theta, v)), dt)
        vn = o.add(o.add(v, vdrift), o.mul(o.mul(o.mul(sigma, sv), sq), zc[1]))
        return [logSn, np.maximum(vn, LD(0.0))]
    aux = [LD(a) for a in tb.aux[_aux_row(tb, k, mut), sl["i"]]]                   # heston.py:161-253 (Andersen QE)
    fuzzy = (sl["flags"] & FLAG_SMOOTHING) != 0
    E, K0, K1, K2, K3, K4, c1, c2 = aux
    if mut == "k1_k2":
        K1, K2 = K2, K1
    m = o.add(theta, o.mul(o.sub(v, theta), E))                                    # :134-143
    s2 = o.add(o.mul(v, c1), c2)                                                   # :123-132
    psi = o.div(s2, o.add(o.mul(m, m), EPS))                                       # :189
    psi_eps = psi if mut == "psi_eps" else o.add(psi, EPS)
    invpsi = o.div(LD(1.0), psi_eps)                                               # :201
    two_inv = LD(2.0) * invpsi
    tm1 = o.sub(two_inv, LD(1.0))
    t = np.maximum(tm1, LD(0.0))                                                   # :202
    with np.errstate(invalid="ignore"):
        root = o.mul(o.sqrt(two_inv), o.sqrt(t))                                   # :203 (NaN for a negative 2 / psi)
    b2 = np.maximum(o.add(tm1, root), LD(0.0))                                     # :203-204
    b = o.sqrt(b2)                                                                 # :206
    a = o.div(m, o.add(LD(1.0), b2))                                               # :207
    bz = o.add(b, zc[1])
    v1 = o.mul(a, o.mul(bz, bz))                                                   # :208
    pp = np.maximum(o.div(o.sub(psi, LD(1.0)), o.add(psi, LD(1.0))), LD(0.0))      # :218-219
    if mut != "p_cap":
        pp = np.minimum(pp, P_CAP)
    omp_raw = o.sub(LD(1.0), pp)
    beta = o.div(omp_raw, o.add(m, EPS))                                           # :220
    omu = o.sub(LD(1.0), u)
    if mut != "omu_floor":
        omu = np.maximum(omu, EPS)                                                 # :222
    omp = np.maximum(omp_raw, EPS)                                                 # :223
    with np.errstate(invalid="ignore", divide="ignore"):
        v_tail = o.div(o.log(o.div(omp, omu)), o.add(beta, EPS))                   # :224
    mu_margin = o.sub(u, pp)
    w_mass = _dot(mu_margin, fuzzy, 0.3, o)                                        # :227
    psi_margin = o.sub(psi, LD(1.5))
    w = _dot(psi_margin, fuzzy, 0.5, o)                                            # :235
    if flip is not None:
        if "u" in flip:
            w_mass = np.where(flip["u"], LD(1.0) - w_mass, w_mass)
        if "psi" in flip:
            w = np.where(flip["psi"], LD(1.0) - w, w)
    v2 = o.mul(w_mass, v_tail)                                                     # :228
    # (a hard indicator multiplies exactly: 0 * x and 1 * x round nothing, the hooks on them only widen the bound a little)
    vn = o.add(o.mul(o.sub(LD(1.0), w), v1), o.mul(w, v2))                         # :236
    var_int = np.maximum(o.add(o.mul(K3, v), o.mul(K4, vn)), LD(0.0))              # :245-246
    vol = o.sqrt(np.maximum(var_int, EPS))                                         # :247
    acc = o.add(o.add(logS, o.mul(rate, dt)), K0)
    acc = o.add(acc, o.mul(K1, v))
    acc = o.add(acc, o.mul(K2, vn))
    logSn = o.add(acc, o.mul(vol, zc[0]))                                          # :251
    mon.update(m=m, psi=psi, p=pp, b=b, psi_eps=psi_eps, margin_u=mu_margin, margin_psi=psi_margin,
               neg_root=np.isfinite(two_inv) & (two_inv < 0))
    return [logSn, vn]


_MAPS = {BS: _bs, VASICEK: _vasicek, HW: _hw, CIRPP: _cirpp, CIRPP_DET: _cirpp_det, S2F: _s2f, HESTON: _heston}
MONITORS = ("psi_eps", "margin_u", "margin_psi")


def _substep(o, tb, k, state, z, u, mut, flip, layout, only=None):
    """one sub-step: z @ L.T (model.py:48), then the per-slot maps.  state: list of n_state long-double rows.
    The slots do not interact: a perturbed run recomputes the slots in `only` alone, every piece (a row of the factor product, a
    slot) at the operation numbers `layout` recorded for it in the base run; the other slots' rows are left as they came."""
    L = tb.chol[tb.chol_idx[k]]
    if mut == "chol_transposed":
        L = L.T
    nz = tb.n_z
    rows = range(nz) if only is None else sorted({r for i in only for r in range(tb.slots[i]["z_off"], tb.slots[i]["z_off"] + SIM_DIM[tb.slots[i]["kind"]])})
    zc = [None] * nz
    for r in rows:
        if only is None:
            layout[(k, "row", r)] = o.n
        else:
            o.n = layout[(k, "row", r)]
        acc = None
        for c in range(nz):
            if L[r, c] == 0.0:
                continue
            term = z[c] if L[r, c] == 1.0 else o.mul(LD(L[r, c]), z[c])
            acc = term if acc is None else o.add(acc, term)
        zc[r] = acc if acc is not None else np.zeros_like(z[0])
    out, mons = list(state), {}
    for i, sl in enumerate(tb.slots):
        so, zo, kind = sl["state_off"], sl["z_off"], sl["kind"]
        if only is None:
            layout[(k, "slot", i)] = o.n
        elif i not in only:
            continue
        else:
            o.n = layout[(k, "slot", i)]
        mon = {}
        args = (o, tb, k, dict(sl, i=i), state[so:so + STATE_DIM[kind]], zc[zo:zo + SIM_DIM[kind]], u, mut, mon)
        new = _heston(*args, flip=flip) if kind == HESTON else _MAPS[kind](*args)
        out[so:so + STATE_DIM[kind]] = new
        mons[i] = mon
    return out, mons


class Advance:
    """value [n_state][n], sens [n_state][n] (multiply by u), nan_mask [n_state][n], and per sub-step j the monitors
    mon[name][j], mon_sens[name][j] (QE only) and floored[slot][j] (CIR++ only)"""


def advance(tb: Tables, k0: int, nsub: int, state, z, u=None, *, mut=None, flip=None, bound=True, per_op=False) -> Advance:
    """state [n_state][n], z [nsub][n_z][n], u [nsub][n] or None: doubles.  flip: {(j, "psi" | "u"): bool mask [n]} takes the other
    branch of a hard QE indicator at sub-step j for the masked paths.  per_op: also sens_ops [n_ops][n_state][n] (float64), the term of
    every operation in sens, and op_names[k] = "<sub-step>.<row r | slot i>.<number within the piece>:<kind>"."""
    st0 = [np.asarray(state[c], dtype=np.float64).astype(LD) for c in range(tb.n_state)]
    if mut == "column_1e-13":
        st0[-1] = st0[-1] * (LD(1.0) + LD(1e-13))
    zl = [[np.asarray(z[j][c], dtype=np.float64).astype(LD) for c in range(tb.n_z)] for j in range(nsub)]
    ul = [np.asarray(u[j], dtype=np.float64).astype(LD) if u is not None else None for j in range(nsub)]
    flips = [{w: m for (jj, w), m in (flip or {}).items() if jj == j} or None for j in range(nsub)]

    # How the bound is computed without re-running everything for every operation.  Two invariants carry it: (1) the slots of a
    # sub-step do not interact — a slot reads its own state columns and its own rows of the factor product, nothing else; (2) the
    # program is straight-line, so an operation has the same number in every run.  The base run records in `layout` the first
    # operation number of every piece (a row of the factor product, a slot) of every sub-step, and the state at the start of every
    # sub-step.  A perturbed run for operation k then starts at k's sub-step from the recorded state, recomputes only the slots k
    # can reach (`only`), and replays each piece at its recorded operation numbers; the other slots' columns are not compared.
    # Paths whose base value is NaN have no bound and are taken out first (the recursion on `keep`).  `per_op` keeps every
    # operation's term so that the harness can name the one that dominates the worst entry.
    layout = {}

    def run(o, j0, st, only):
        mons = []
        for j in range(j0, nsub):
            st, mo = _substep(o, tb, k0 + j, st, zl[j], ul[j], mut, flips[j], layout, only)
            mons.append(mo)
        return st, mons

    # base run, remembering the state at the start of every sub-step and the operation numbers of every piece
    o, starts, st, base_mons = Ops(), [], st0, []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(nsub):
            starts.append(st)
            st, mo = _substep(o, tb, k0 + j, st, zl[j], ul[j], mut, flips[j], layout)
            base_mons.append(mo)
    n_ops = o.n
    # (sub-step, slots it reaches, first op, one past its last op) of every piece, in operation order
    marks = sorted((first, key) for key, first in layout.items())
    pieces = []
    for q, (first, (kk, what, idx)) in enumerate(marks):
        last = marks[q + 1][0] if q + 1 < len(marks) else n_ops
        owners = [idx] if what == "slot" else [i for i, sl in enumerate(tb.slots) if sl["z_off"] <= idx < sl["z_off"] + SIM_DIM[sl["kind"]]]
        pieces.append((kk - k0, owners, first, last, f"{'factor row' if what == 'row' else 'slot'} {idx}"))
    res = Advance()
    res.value = np.stack(st)
    res.n_ops = n_ops
    qe = [i for i, sl in enumerate(tb.slots) if sl["kind"] == HESTON and tb.scheme == SCHEME_QE]
    res.mon = {name: np.stack([base_mons[j][qe[0]][name] for j in range(nsub)]) for name in MONITORS + ("neg_root",)} if qe else {}
    res.floored = {i: np.stack([base_mons[j][i]["floored"] for j in range(nsub)]) for i, sl in enumerate(tb.slots) if sl["kind"] == CIRPP}
    in_nan = np.isnan(np.stack(st0)).any(axis=0)
    res.nan_mask = np.isnan(res.value) & ~in_nan[None]
    if not bound:
        return res
    keep = ~np.isnan(res.value).any(axis=0)
    if not keep.all():
        # the bound of the finite paths alone (a NaN entry has none; long-double arithmetic on NaN operands is also very slow)
        res.sens = np.zeros_like(res.value)
        res.mon_sens = {name: np.zeros_like(res.mon[name]) for name in MONITORS} if qe else {}
        if per_op:
            res.sens_ops = np.zeros((n_ops,) + res.value.shape)
        if keep.any():
            sub = advance(tb, k0, nsub, [np.asarray(state[c])[keep] for c in range(tb.n_state)],
                          [[np.asarray(z[j][c])[keep] for c in range(tb.n_z)] for j in range(nsub)],
                          [np.asarray(u[j])[keep] for j in range(nsub)] if u is not None else None, mut=mut,
                          flip={key: m[keep] for key, m in flip.items()} if flip else None, per_op=per_op)
            res.op_names = getattr(sub, "op_names", None)
            if per_op:
                res.sens_ops[:, :, keep] = sub.sens_ops
            res.sens[:, keep] = sub.sens
            for name in res.mon_sens:
                res.mon_sens[name][:, keep] = sub.mon_sens[name]
        return res
    sens = np.zeros_like(res.value)
    if per_op:
        sens_ops = np.zeros((n_ops,) + res.value.shape)
        res.sens_ops = sens_ops
        res.op_names = {}
        for j0, owners, first, last, what in pieces:
            for k in range(first, last):
                res.op_names[k] = f"sub-step {j0}, {what}, operation {k - first}: {o.kinds[k]}"
    msens = {name: np.zeros_like(res.mon[name]) for name in MONITORS} if qe else {}

    def dev(pert, base):
        with np.errstate(invalid="ignore"):
            d = np.abs(pert - base) / D_FD
        return np.where(np.isnan(d), np.where(np.isnan(base), LD(0.0), LD(np.inf)), d)

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j0, owners, first, last, _what in pieces:
            cols = [c for i in owners for c in range(tb.slots[i]["state_off"], tb.slots[i]["state_off"] + STATE_DIM[tb.slots[i]["kind"]])]
            for k in range(first, last):
                worst = np.zeros((len(cols),) + sens.shape[1:], dtype=LD)
                mworst = {name: np.zeros_like(msens[name]) for name in msens}
                for sign in (1.0, -1.0):
                    stp, mo = run(Ops(k, sign * D_FD), j0, starts[j0], owners)
                    worst = np.maximum(worst, dev(np.stack([stp[c] for c in cols]), res.value[cols]))
                    for name in msens:
                        for jj in range(j0, nsub):
                            mworst[name][jj] = np.maximum(mworst[name][jj], dev(mo[jj - j0][qe[0]][name], res.mon[name][jj]))
                sens[cols] += worst
                if per_op:
                    sens_ops[k][cols] = worst
                for name in msens:
                    msens[name] += mworst[name]
    res.sens, res.mon_sens = sens, msens
    return res


def self_start(tb: Tables, n: int):
    """the model's own start state for n paths [n_state][n]"""
    return np.tile(tb.init_state[:, None], (1, n))


class Report:
    def __init__(self):
        self.worst, self.failures, self.dominant = {}, [], {}
        self.near_branch = self.ill_conditioned = self.finite_path_steps = self.entries = self.floored = self.nan_entries = 0

    def merge(self, other):
        for k, v in other.worst.items():
            if v > self.worst.get(k, 0.0) and k in other.dominant:
                self.dominant[k] = other.dominant[k]
            self.worst[k] = max(self.worst.get(k, 0.0), v)
        self.failures += other.failures
        for a in ("near_branch", "ill_conditioned", "finite_path_steps", "entries", "floored", "nan_entries"):
            setattr(self, a, getattr(self, a) + getattr(other, a))
        return self

    def assert_ok(self, tag=""):
        assert not self.failures, (tag, self.failures[:5], len(self.failures))

    def __str__(self):
        w = "  ".join(f"{k} {v:.3f}" for k, v in sorted(self.worst.items()))
        if self.dominant:
            w += " [" + "; ".join(f"{k}: {v}" for k, v in sorted(self.dominant.items())) + "]"
        return (f"worst ratio: {w} | entries {self.entries}, near-branch {self.near_branch}, ill-conditioned {self.ill_conditioned} of "
                f"{self.finite_path_steps} finite path-steps, floored {self.floored}, NaN {self.nan_entries}")


def check_paths(tb: Tables, paths, draws, u_round, *, mut=None, transitions=None, n_edge=0, explain=False) -> Report:
    """paths [n_dates][n_state][n] (doubles, the checked implementation's stored states).  draws(k) -> (z [n_z][n], u [n] | None): the
    uncorrelated normals and the uniform of sub-step k for the same paths.  Every transition between stored dates is advanced in
    the reference from the implementation's own state at its start and the state at its end must lie within u_round * sens; the
    NaN pattern must be equal.

    Hard QE: a path-step whose indicator margin lies inside the margin's own bound is counted in near_branch and must match one
    of the two branches.  Smoothed QE: an entry whose bound exceeds 1e-6 |value| (paths from n_edge on), or whose psi + eps changes
    sign inside its bound, is counted in ill_conditioned and left out.  Every other map: nothing is left out.  The caller asserts the caps."""
    paths = np.asarray(paths, dtype=np.float64)
    rep = Report()
    qe = tb.scheme == SCHEME_QE
    smooth = qe and (tb.slots[0]["flags"] & FLAG_SMOOTHING) != 0
    uld = LD(u_round)
    for (d0, d1, k0, nsub) in (transitions if transitions is not None else tb.transitions()):
        dr = [draws(k0 + j) for j in range(nsub)]
        z = [d[0] for d in dr]
        u = [d[1] for d in dr] if dr[0][1] is not None else None
        start = paths[d0] if d0 >= 0 else self_start(tb, paths.shape[2])
        ref = advance(tb, k0, nsub, start, z, u, mut=mut, per_op=explain)
        got = paths[d1].astype(LD)
        got_nan, ref_nan = np.isnan(paths[d1]), np.isnan(ref.value)
        if not np.array_equal(got_nan, ref_nan):
            rep.failures.append(("NaN pattern", d0, d1, int((got_nan != ref_nan).sum())))
        fin = ~(got_nan | ref_nan)
        rep.nan_entries += int(ref_nan.sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(got - ref.value)
            bnd = uld * ref.sens
            ratio = np.where(err == 0, LD(0.0), err / bnd)          # (an exact entry has bound 0 and must be reproduced exactly)
        ratio = np.where(fin, ratio, LD(0.0))
        skip = np.zeros(paths.shape[2], dtype=bool)
        # a perturbed run that is NaN where the base run is not gives an infinite bound, under which any value would pass: such an
        # entry counts as ill-conditioned under smoothed QE (against its cap, the edge block included) and fails everywhere else
        unbounded = (~np.isfinite(ref.sens) & fin).any(axis=0)
        if unbounded.any() and not smooth:
            rep.failures.append(("infinite bound", "dates", d0, d1, "paths", int(unbounded.sum())))
        if qe:
            fin_ps = fin.all(axis=0)
            rep.finite_path_steps += int(fin_ps.sum()) * nsub
            if smooth:
                with np.errstate(invalid="ignore"):
                    ill = (bnd > LD(1e-6) * np.abs(ref.value)).any(axis=0)
                    # (the edge states cancel v' to nothing on purpose, b + z1 = 0: their bound is large against the value for
                    #  that reason and not for a pole; they are checked like every other entry)
                    ill[:n_edge] = False
                    ill |= unbounded
                    ill |= (np.abs(ref.mon["psi_eps"]) <= uld * ref.mon_sens["psi_eps"]).any(axis=0)
                ill &= fin_ps
                rep.ill_conditioned += int(ill.sum())
                skip = ill
            else:
                with np.errstate(invalid="ignore"):
                    near = {w: np.abs(ref.mon["margin_" + w]) <= uld * ref.mon_sens["margin_" + w] for w in ("u", "psi")}
                any_near = (near["u"] | near["psi"]).any(axis=0) & fin_ps
                if any_near.any():
                    # never merely skipped: the entry must match the branch on the other side of the margin
                    flip = {(j, w): near[w][j] for j in range(nsub) for w in ("u", "psi") if near[w][j].any()}
                    alt = advance(tb, k0, nsub, start, z, u, mut=mut, flip=flip)
                    # (an indicator whose two sides give the same state decides nothing: u against p while psi < 1.5 weighs the
                    #  tail branch with 0 — the edge states at psi = 1, where p is 5e-10 +- 1e-14, are of this kind)
                    any_near &= (alt.value != ref.value).any(axis=0)
                    rep.near_branch += int(any_near.sum())
                    with np.errstate(invalid="ignore", divide="ignore"):
                        e2 = np.abs(got - alt.value)
                        r2 = np.where(e2 == 0, LD(0.0), e2 / (uld * alt.sens))
                    ratio = np.where(any_near[None], np.minimum(ratio, np.where(fin, r2, LD(0.0))), ratio)
        for i, sl in enumerate(tb.slots):
            so, sd = sl["state_off"], STATE_DIM[sl["kind"]]
            r = ratio[so:so + sd][:, ~skip]
            name = tb.map_name(i)
            if explain and r.size and float(r.max()) > rep.worst.get(name, 0.0):
                # the operation with the largest term in the bound of the worst entry
                c, q = np.unravel_index(int(np.argmax(r)), r.shape)
                col = np.flatnonzero(~skip)[q]
                terms = ref.sens_ops[:, so + c, col]
                k = int(np.argmax(terms))
                rep.dominant[name] = f"{ref.op_names[k]} ({float(terms[k] / terms.sum()):.0%} of the bound; column {int(c)})"
            rep.worst[name] = max(rep.worst.get(name, 0.0), float(r.max()) if r.size else 0.0)
            rep.entries += int(fin[so:so + sd][:, ~skip].sum())
            bad = np.argwhere(~(r <= 1.0))
            for c, q in bad[:3]:
                col = np.flatnonzero(~skip)[q]
                rep.failures.append((name, "dates", d0, d1, "column", so + int(c), "path", int(col), "ratio", float(r[c, q]),
                                     "got", float(paths[d1, so + c, col]), "ref", float(ref.value[so + c, col])))
            if len(bad) > 3:
                rep.failures.append((name, "dates", d0, d1, "entries outside the bound", len(bad)))
        for i, fl in ref.floored.items():
            # how many entries the CIR++ floor caught: the state stored after the last sub-step is 1e-12 exactly where the reference's is
            rep.floored += int(fl.sum())
            got_floored = paths[d1, tb.slots[i]["state_off"]] == 1e-12
            if not np.array_equal(got_floored, fl[-1]):
                rep.failures.append(("CIR++ floor", "dates", d0, d1, "floored", int(got_floored.sum()), "reference", int(fl[-1].sum())))
    return rep
