"""Models, start states and draws of the step-level pin (tests/step_reference.py): shared by the CPU suite, which drives the
oracle backend through the harness (tests/test_step_reference.py), and the GPU suite, which drives every kernel route
(tests/test_step_kernels.py).

Shapes: n = 4097 paths (16 full blocks and one lane; an odd tail for two paths per lane), five stored dates on the non-uniform
grid GRID (distinct dt: distinct covariance factors and aux rows per step under ANALYTICAL), 1 or 3 sub-steps per interval.
Parameter sets: seeded draws from the ranges of test_hip_parity.test_random_model_parameters_gpu_vs_oracle, four per step map,
and the 24 sets of test_heston_qe_random_parameters_gpu_vs_oracle, of which QE_HARD / QE_SMOOTH select by what the oracle does
with them (test_step_reference.test_qe_sets_are_what_they_are_chosen_for)."""
import numpy as np

import cases
import step_reference as sr
from mcx.common.enums import SimulationScheme as SS
from mcx.models.black_scholes import BlackScholesModel
from mcx.models.black_scholes_multi import BlackScholesMulti
from mcx.models.cirpp import CIRPPModel
from mcx.models.heston import HestonModel
from mcx.models.hull_white import HullWhiteModel
from mcx.models.model_config import ModelConfig
from mcx.models.schwartz_two_factor import SchwartzTwoFactorModel
from mcx.models.vasicek import VasicekModel
from mcx.plan import SimPlan

GRID = np.array([0.0, 0.1, 0.35, 0.4, 1.4])
N = 4097
EDGE = 320                       # paths of the injected route that start from the edge states
OFFSET_BIG = 2 ** 33 + 12345
A, E, Q = SS.ANALYTICAL, SS.EULER, SS.QE


def _lu(rng, lo, hi):
    return float(10.0 ** rng.uniform(np.log10(lo), np.log10(hi)))


def bs(rng):
    return BlackScholesModel(0, _lu(rng, 1.0, 1e3), float(rng.uniform(-0.02, 0.1)), _lu(rng, 0.01, 1.5))


def vas(rng, asset_id=None):
    return VasicekModel(0.0, float(rng.uniform(-0.01, 0.08)), float(rng.uniform(-0.01, 0.1)), _lu(rng, 1e-3, 5.0), _lu(rng, 1e-4, 0.1),
                        asset_id=asset_id)


def cir(rng, deterministic=False):
    kappa, theta = _lu(rng, 0.02, 3.0), _lu(rng, 1e-3, 0.2)
    vol = float(rng.uniform(0.05, 0.95)) * np.sqrt(2 * kappa * theta)
    return CIRPPModel(0.0, "cp", cases.HAZARDS, kappa=kappa, theta=theta, volatility=vol, y0=_lu(rng, 1e-9, 0.05), deterministic=deterministic)


def hw(rng, a=None):
    ts = np.linspace(0.0, 25.0, 26)
    f = 0.03 + 0.02 * np.sin(ts / float(rng.uniform(2.0, 9.0))) + float(rng.uniform(-0.01, 0.02))
    return HullWhiteModel(0.0, float(f[0]), list(f), list(np.gradient(f, ts)), _lu(rng, 1e-2, 2.0) if a is None else a, _lu(rng, 1e-3, 0.05),
                          curve_times=list(ts))


def s2f(rng):
    ts = [0.0, 0.5, 1.0, 2.0, 5.0, 25.0]
    return SchwartzTwoFactorModel(0.0, ts, [_lu(rng, 10.0, 90.0) for _ in ts], rate=float(rng.uniform(0.0, 0.06)),
                                  short_term_mean_reversion=_lu(rng, 1e-3, 5.0), short_term_vol=_lu(rng, 0.02, 0.8),
                                  long_term_drift=float(rng.uniform(-0.05, 0.05)), long_term_vol=_lu(rng, 0.01, 0.4),
                                  rho=float(rng.uniform(-0.9, 0.9)))


def multi(rng):
    a = rng.normal(size=(4, 4))
    c = a @ a.T
    d = np.sqrt(np.diag(c))
    ids = [f"a{k}" for k in range(4)]
    corr = 0.5 * np.eye(4) + 0.5 * c / np.outer(d, d)
    return BlackScholesMulti(0.0, float(rng.uniform(0.0, 0.06)), ids, [_lu(rng, 10.0, 500.0) for _ in ids], [_lu(rng, 0.02, 0.9) for _ in ids], corr)


def vas_cir(rng, rho=None):
    rho = float(rng.uniform(-0.95, 0.95)) if rho is None else rho
    return ModelConfig([vas(rng, "ir"), cir(rng)], inter_asset_correlation_matrix=np.array([rho]))


def bs_vas_cirdet(rng):
    eq = BlackScholesModel(0.0, _lu(rng, 1.0, 1e3), float(rng.uniform(-0.02, 0.1)), _lu(rng, 0.01, 1.5), asset_id="equity")
    return ModelConfig([eq, vas(rng, "rates"), cir(rng, True)], inter_asset_correlation_matrix=[np.array([float(rng.uniform(-0.5, 0.5))])] * 3)


def multi_cir(rng):
    return ModelConfig([multi(rng), cir(rng)], inter_asset_correlation_matrix=[rng.uniform(-0.15, 0.15, size=(4, 1))])


def heston_euler(rng):
    return HestonModel(0.0, 100.0, float(rng.uniform(-0.02, 0.08)), _lu(rng, 1e-2, 1.0), float(rng.uniform(-0.95, 0.95)), _lu(rng, 1e-2, 10.0),
                       _lu(rng, 1e-4, 0.3), _lu(rng, 1e-4, 0.3))


def qe_sweep_sets():
    """the 24 parameter sets of test_hip_parity.test_heston_qe_random_parameters_gpu_vs_oracle (same generator, same order)"""
    rng = np.random.default_rng(20261005)
    out = []
    for case in range(24):
        v0 = float(10.0 ** rng.uniform(-6.0, -0.5))
        theta = float(10.0 ** rng.uniform(-6.0, -0.5))
        kappa = float(10.0 ** rng.uniform(-2.0, 1.2))
        sigma = float(10.0 ** rng.uniform(-2.0, 0.5))
        rho = float(rng.uniform(-0.95, 0.95))
        rate = float(rng.uniform(-0.02, 0.08))
        horizon = float(10.0 ** rng.uniform(-1.0, 1.0))
        steps = int(rng.integers(1, 6))
        out.append(dict(v0=v0, theta=theta, kappa=kappa, sigma=sigma, rho=rho, rate=rate, horizon=horizon, steps=steps))
    return out


# One set beyond the sweep: p reaches its cap 1 - 1e-6 only for psi > 2e6 with m^2 well above the eps of psi's denominator, which
# takes sigma^2 / (2 kappa theta) > 2e6 AND kappa theta dt > 1e-5 — a vol-of-vol of 70.  (The sweep's largest psi is 1.5e6.)  The
# cap then decides a state only where u > p, one draw in a million: the edge states u = 1 - 2^-54 and u = p (1 + 1e-9).
QE_CAP = 24


def heston_qe(case: int, smoothing: bool):
    q = qe_sweep_sets()[case] if case != QE_CAP else dict(rate=0.02, sigma=70.0, rho=-0.5, kappa=1.0, theta=1e-3, v0=1e-3)
    m = HestonModel(0.0, 100.0, q["rate"], q["sigma"], q["rho"], q["kappa"], q["theta"], q["v0"])
    m.perform_smoothing = smoothing
    return m


# (set of the sweep, sub-steps per interval) by what the oracle does with them on GRID with n = 4097 injected draws — share of path-steps
# on the tail side of psi = 1.5: none for 3 and 13, all for 10 and 12, 42 % / 58 % / 24 % / 47 % for 1, 9, 16, 21
# (test_step_reference.test_qe_sets_are_what_they_are_chosen_for)
QE_HARD = {"quadratic": [(3, 1), (13, 1)], "tail": [(10, 1), (12, 1)], "mixed": [(1, 1), (9, 1), (16, 3), (21, 1)]}
# smoothed sets whose variance goes negative (4.2 % - 17.7 % of the stored entries NaN on the oracle, edge states included)
QE_SMOOTH = [(1, 1), (7, 1), (14, 1), (21, 3)]


def _case_list():
    """(id, builder(rng) -> model, scheme, sub-steps, seed) of every non-QE case: four seeded parameter sets per step map"""
    out = []
    def add(name, build, schemes, reps=4):
        for scheme in schemes:
            for rep in range(reps):
                out.append((f"{name}-{scheme.name.lower()}-{rep}", build, scheme, 1 if rep % 2 == 0 else 3, 1000 * len(out) + rep))
    add("bs", bs, (A, E)); add("vasicek", vas, (A, E)); add("hull_white", hw, (A, E)); add("s2f", s2f, (A, E)); add("cirpp", cir, (E,))
    add("bs_vas_cirdet", bs_vas_cirdet, (E,)); add("heston", heston_euler, (E,))
    return out


# K1 with injected draws and per-path start states: all twelve step maps (the QE sets come from QE_HARD / QE_SMOOTH)
INJECTED = _case_list()
# a dt in {1e-4, 20} on the first interval (Vasicek, Hull-White); exponent arguments of +-12 (Black-Scholes ANALYTICAL, sigma sqrt(dt) = 1.42);
# a CIR++ whose floor engages in the edge block
INJECTED_SPECIAL = (
    [(f"vasicek-{sch.name.lower()}-adt{adt:g}", (lambda rng, a=adt / 0.1: VasicekModel(0.0, 0.03, 0.05, a, 0.01)), sch, 1, 77) for sch in (A, E) for adt in (1e-4, 20.0)]
    + [(f"hull_white-{sch.name.lower()}-adt{adt:g}", (lambda rng, a=adt / 0.1: hw(rng, a)), sch, 1, 78) for sch in (A, E) for adt in (1e-4, 20.0)]
    + [("bs-analytical-exp12", (lambda rng: BlackScholesModel(0, 100.0, 0.03, 4.5)), A, 1, 79),
       # a volatility at 0.9 of the Feller bound: z = -8.5 takes y = 0.05 (and, later, many a path) below the floor
       ("cirpp-euler-floor", (lambda rng: CIRPPModel(0.0, "cp", cases.HAZARDS, kappa=0.5, theta=0.02, volatility=0.9 * np.sqrt(0.02), y0=1e-3)), E, 1, 80)])


def _philox_list():
    out = []
    def add(name, build, schemes, sig, reps=4):
        for scheme in schemes:
            for rep in range(reps):
                out.append((f"{name}-{scheme.name.lower()}-{rep}", build, scheme, 1 if rep % 2 == 0 else 3, 5000 + 1000 * len(out) + rep, sig[scheme]))
    add("bs", bs, (A, E), {A: "BS_A", E: "BS_E"}); add("vasicek", vas, (A, E), {A: "VAS_A", E: "VAS_E"})
    add("vas_cir+0.95", lambda rng: vas_cir(rng, 0.95), (E,), {E: "VAS_CIR_E"}, 2); add("vas_cir-0.95", lambda rng: vas_cir(rng, -0.95), (E,), {E: "VAS_CIR_E"}, 2)
    add("heston", heston_euler, (E,), {E: "HESTON_E"}); add("bs_vas_cirdet", bs_vas_cirdet, (E,), {E: "BS_VAS_CIRDET_E"})
    g = {A: "GENERIC", E: "GENERIC"}
    add("hull_white", hw, (A, E), g); add("s2f", s2f, (A, E), g); add("cirpp", cir, (E,), g); add("multi", multi, (A, E), g, 2); add("multi_cir", multi_cir, (E,), g, 2)
    return out


# K1 with Philox draws: (id, builder, scheme, sub-steps, seed, the signature mcx_sim_describe must report)
PHILOX = _philox_list()


def build_model(case):
    return case[1](np.random.default_rng(case[4]))


# ---- runs ---------------------------------------------------------------------------------------------------------------------
class Run:
    """tables, the stored paths [n_dates][n_state][n] (numpy) and draws(k) of one run"""

    def __init__(self, plan, paths, draws):
        self.plan, self.tb, self.paths, self.draws = plan, sr.Tables(plan), paths, draws


def start_states(plan, n, rng):
    """per-path start states around the model's own: positive columns scaled by e^(0.3 N), the others shifted"""
    st = np.tile(np.asarray(plan.init_state, dtype=np.float64)[:, None], (1, n))
    tb = sr.Tables(plan)
    for sl in tb.slots:
        so, kind = sl["state_off"], sl["kind"]
        if kind in (sr.BS, sr.CIRPP, sr.CIRPP_DET):
            st[so] *= np.exp(0.3 * rng.standard_normal(n))
        elif kind == sr.HESTON:
            st[so] += 0.2 * rng.standard_normal(n)
            st[so + 1] *= np.exp(rng.standard_normal(n))
        elif kind in (sr.VASICEK, sr.HW):
            st[so] += 0.02 * rng.standard_normal(n)
            st[so + 1] = 0.05 * rng.standard_normal(n)
        elif kind == sr.S2F:
            st[so + 1], st[so + 2] = 0.2 * rng.standard_normal(n), 0.1 * rng.standard_normal(n)
            st[so] = st[so] + st[so + 1] + st[so + 2]
        if kind == sr.CIRPP:
            st[so + 1] = 0.01 * rng.random(n)
    return st


def edge_states(plan, st, z, u):
    """overwrite the first paths' start states and first-sub-step draws with the edge states of every slot kind (in place);
    returns the number of paths used"""
    tb = sr.Tables(plan)
    used, n = 0, st.shape[1]
    for i, sl in enumerate(tb.slots):
        so, zo, kind, p = sl["state_off"], sl["z_off"], sl["kind"], sl["p"]
        if n < 256:
            break                                          # (the one tiny run checks the launch shape, not the edge states)
        if kind == sr.CIRPP:
            # y in ys x correlated normal in zs for 15 paths, then 15 paths that keep their random normal, and so on.  The Cholesky
            # factor mixes the slots: the uncorrelated normal is solved so that the CORRELATED one is the target exactly
            ys, zs = [0.0, 1e-12, 1e-9, 0.05, -1e-4], [-8.5, 8.5, 0.0]
            cnt = 256
            L = tb.chol[tb.chol_idx[0]]
            for q in range(cnt):
                st[so, q] = ys[q % 5]
                if (q // 15) % 2 == 0:
                    z[0, zo, q] = (zs[(q // 5) % 3] - float(np.dot(L[zo, :zo], z[0, :zo, q]))) / L[zo, zo]
            used = max(used, cnt)
        elif kind == sr.BS and tb.scheme == sr.SCHEME_ANALYTICAL and len(tb.slots) == 1:
            L00 = tb.chol[tb.chol_idx[0]][0, 0]
            for q in range(64):
                z[0, 0, q] = (12.0 if q % 2 else -12.0) / L00 * (1.0 + 0.01 * (q // 2))      # exponent arguments of about +-12
            used = max(used, 64)
        elif kind == sr.HESTON:
            theta = p[5]
            vs = [0.0, 1e-30, 10.0] + [theta * 10.0 ** k for k in range(-6, 4)]
            if tb.scheme == sr.SCHEME_EULER:
                vs += [-1e-4]
                zs = [0.0, 8.5, -8.5]
                for q in range(EDGE):
                    st[so + 1, q] = vs[q % len(vs)]
                    z[0, 1, q] = zs[(q // len(vs)) % 3]
                used = max(used, EDGE)
                continue
            # v with psi(v) = 1, 1.5, 2 (each (1 +- 1e-9)): psi (m^2 + eps) = s2 is a quadratic in v, solved in long double
            aux = tb.aux[0, i]
            Ee, c1, c2 = sr.LD(aux[0]), sr.LD(aux[6]), sr.LD(aux[7])
            th = sr.LD(theta)
            for target in (1.0, 1.5, 2.0):
                for rel in (-1e-9, 1e-9):
                    ps = sr.LD(target) * (1 + sr.LD(rel))
                    m0 = th * (1 - Ee)
                    qa, qb, qc = ps * Ee * Ee, 2 * ps * Ee * m0 - c1, ps * (m0 * m0 + sr.EPS) - c2
                    disc = qb * qb - 4 * qa * qc
                    if disc >= 0:
                        for root in ((-qb + np.sqrt(disc)) / (2 * qa), (-qb - np.sqrt(disc)) / (2 * qa)):
                            if root > 0:
                                vs.append(float(root))
                                break
            vs = np.array(vs)
            t = sr.qe_terms(tb, 0, vs, i)
            L = tb.chol[tb.chol_idx[0]]
            combos = [(a, b) for a in range(4) for b in range(4)]
            cnt = 0
            for ci, (ui, zi) in enumerate(combos):
                for vi in range(len(vs)):
                    q = ci * len(vs) + vi
                    if q >= EDGE:
                        break
                    st[so + 1, q] = vs[vi]
                    pp = float(t["p"][vi])
                    u[0, q] = [2.0 ** -54, 1.0 - 2.0 ** -54, pp * (1 - 1e-9) if pp > 0 else 0.25, pp * (1 + 1e-9) if pp > 0 else 0.75][ui]
                    target = [0.0, 8.5, -8.5, -float(t["b"][vi])][zi]
                    z[0, 1, q] = (target - L[1, 0] * z[0, 0, q]) / L[1, 1]
                    cnt = q + 1
            used = max(used, cnt)
    return used


def run_injected(be, model, scheme, nsub, n, seed, edges=False, path_offset=0):
    """the route with injected draws and per-path start states (generate_paths(init_state=, inject_z=, inject_u=))"""
    plan = SimPlan(model, GRID, scheme, nsub)
    rng = np.random.default_rng(seed)
    st = start_states(plan, n, rng)
    z = rng.standard_normal((plan.n_steps, plan.n_z, n))
    u = rng.random((plan.n_steps, n)) if plan.n_uniform else None
    n_edge = edge_states(plan, st, z, u) if edges else 0
    sim = be.sim_create(plan)
    out = be.generate_paths(sim, 0, path_offset, n, inject_z=be.from_numpy(z), inject_u=be.from_numpy(u) if u is not None else None,
                            init_state=be.from_numpy(st))
    be.synchronize()
    run = Run(plan, out.cpu().numpy(), lambda k: (z[k], u[k] if u is not None else None))
    run.n_edge, run.start, run.sim = n_edge, st, sim
    return run


def philox_draws(hip, plan, seed, path_offset, n, bits=7):
    """draws(k) of a Philox route from the library's own helpers: rng_draws -> box_muller with the route's table size; the QE
    uniform is the first uniform of draw (n_z + 1) / 2"""
    def draws(k):
        nz = plan.n_z
        z = np.empty((nz, n))
        for q in range((nz + 1) // 2):
            words, _u, _z = hip.rng_draws(seed, path_offset, n, k, q)
            _u2, zz = hip.box_muller(words, bits)
            zz = zz.cpu().numpy()
            z[2 * q] = zz[0]
            if 2 * q + 1 < nz:
                z[2 * q + 1] = zz[1]
        u = None
        if plan.n_uniform:
            _w, uu, _z = hip.rng_draws(seed, path_offset, n, k, (nz + 1) // 2)
            u = uu.cpu().numpy()[0]
        return z, u
    return draws


def run_philox(hip, model, scheme, nsub, n, path_offset=0, seed=43):
    from mcx.engine.engine import MonteCarloEngine
    eng = MonteCarloEngine(GRID, scheme, model, n, nsub, backend=hip, path_offset=path_offset)
    paths = eng.generate_paths_native().cpu().numpy()
    run = Run(eng.plan, paths, philox_draws(hip, eng.plan, eng.seed, path_offset, n))
    run.sim = eng.sim
    return run


# ---- the draws of the CPU oracle, without the oracle ---------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on numpy uint64 arrays holding 32-bit words (Salmon et al., SC'11)"""
    M0, M1, MASK = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & MASK, (k1 + np.uint64(0xBB67AE85)) & MASK
    return c0, c1, c2, c3


def host_draws(plan, seed, path_offset, n):
    """draws(k) as the CPU oracle makes them (oracle/mcx_oracle.c orc_draw: the counter (path, step, draw), two 53-bit uniforms,
    the libm Box-Muller pair), in numpy: the uniforms are exact, the normals agree with the oracle's to a few ulp"""
    path = np.uint64(path_offset) + np.arange(n, dtype=np.uint64)
    lo, hi = path & np.uint64(0xFFFFFFFF), path >> np.uint64(32)

    def pair(k, q):
        w = philox4x32_10(lo, hi, np.uint64(k), np.uint64(q), seed & 0xFFFFFFFF, seed >> 32)
        ua = (((w[1] << np.uint64(32)) | w[0]) >> np.uint64(11)).astype(np.float64) + 0.5
        ub = (((w[3] << np.uint64(32)) | w[2]) >> np.uint64(11)).astype(np.float64) + 0.5
        ua, ub = ua * 2.0 ** -53, ub * 2.0 ** -53
        r, th = np.sqrt(-2.0 * np.log(ua)), 6.283185307179586476925 * ub
        return ua, r * np.cos(th), r * np.sin(th)

    def draws(k):
        nz = plan.n_z
        z = np.empty((nz, n))
        for q in range((nz + 1) // 2):
            _ua, z0, z1 = pair(k, q)
            z[2 * q] = z0
            if 2 * q + 1 < nz:
                z[2 * q + 1] = z1
        return z, (pair(k, (nz + 1) // 2)[0] if plan.n_uniform else None)
    return draws


def qe_exposed_share(plan, paths, draws, smoothing):
    """From the ORACLE's paths alone: the share of stored entries downstream of a path-step at which a last-bits difference can
    change the state by more than rounding.  Hard regime: a branch margin (u - p or psi - 1.5) within 1e-9.  Smoothed regime:
    psi + eps within 1e-6 relative of its zero, the pole of 1 / (psi + eps).  The margins come from the long-double reference
    advanced from the oracle's stored states."""
    tb = sr.Tables(plan)
    n_dates, n = paths.shape[0], paths.shape[2]
    first = np.full(n, n_dates)
    for d0, d1, k0, ns in tb.transitions():
        dr = [draws(k0 + j) for j in range(ns)]
        a = sr.advance(tb, k0, ns, paths[d0] if d0 >= 0 else sr.self_start(tb, n), [d[0] for d in dr], [d[1] for d in dr], bound=False)
        with np.errstate(invalid="ignore"):
            if smoothing:
                hit = (np.abs(a.mon["psi_eps"]) <= 1e-6 * np.abs(a.mon["psi_eps"] - sr.EPS)).any(axis=0)
            else:
                hit = ((np.abs(a.mon["margin_u"]) <= 1e-9) | (np.abs(a.mon["margin_psi"]) <= 1e-9)).any(axis=0)
        first[hit] = np.minimum(first[hit], d1)
    return float((n_dates - first).sum()) / (n_dates * n)
