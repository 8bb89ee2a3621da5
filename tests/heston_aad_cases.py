"""Sensitivities of Heston books that go through exposures or exercise: the cases behind tests/golden/heston_*_aad.npz, recorded from
the reference's autograd by tests/golden/gen_heston_aad_golden.py.  `lib` is the namespace the classes are taken from: tests/cases.py
(mcx) by default, the reference's own classes when the generator records the fixtures."""
import types

import numpy as np

# [spot, rate, sigma_v, rho, kappa, theta, v0] in the constructor's order
FELLER = (100.0, 0.03, 0.3, -0.6, 2.0, 0.06, 0.05)            # 2 kappa theta = 0.24 > sigma_v^2 = 0.09
HIGHPSI = (100.0, 0.02, 1.2, -0.5, 0.5, 0.02, 0.02)           # the parameters of cases.heston_highpsi: psi up to sigma_v^2 / (2 kappa theta) = 72


def _lib(lib):
    if lib is None:
        import cases as lib
    return lib


def american(lib=None, params=FELLER):
    """an American put with 8 exercise dates (k / 8, k = 0 .. 7), PV and EPE on 5 of them: 7 intervals, so that the recorded draws
    of 512 + 512 paths stay below the size of the largest committed fixture"""
    lib = _lib(lib)
    model = lib.HestonModel(0.0, *params)
    prod = lib.AmericanOption(lib.Equity(), 0.875, 8, 100.0, lib.OptionType.PUT)
    prod.name = "american_put"
    return [lib.NettingSet(name="american", products=[prod])], model, \
        lib.RiskMetrics([lib.PVMetric(), lib.EPEMetric()], exposure_timeline=np.array([0.0, 0.25, 0.5, 0.75, 0.875]))


def bermudan_highpsi(lib=None):
    return american(lib, HIGHPSI)


def netting(lib=None):
    """a call and a put with different maturities in one netting set.  Short maturities: the margin condition of the fixtures asks
    that no Euler path of 512 + 512 reaches the variance floor, which over half a year and more happens under every seed (40 tried).
    (REGRESSION_DEGREE has the consequence for the regression basis)"""
    lib = _lib(lib)
    model = lib.HestonModel(0.0, *FELLER)
    call = lib.EuropeanOption(lib.Equity(), 0.15, 95.0, lib.OptionType.CALL)
    call.name = "call"
    put = lib.EuropeanOption(lib.Equity(), 0.25, 105.0, lib.OptionType.PUT)
    put.name = "put"
    mets = [lib.PVMetric(), lib.EPEMetric(), lib.ENEMetric(), lib.PFEMetric(0.95), lib.EEPEMetric()]
    return [lib.NettingSet(name="book", products=[call, put])], model, \
        lib.RiskMetrics(mets, exposure_timeline=np.array([0.0, 0.05, 0.1, 0.15, 0.25]))


# PolyomialRegression(degree) of the cases.  Degree 1, not the controller's default 2, because on the quadratic basis the REFERENCE'S TAPE
# is what misses the bound of check_lsm_sensitivities, not the code under test.  The fixtures also record the reference's results and
# gradients of the same draws with degree 2 (deg2_*), and tests/test_tangent_heston_host.py holds them against the host restatement of
# the whole pipeline (tests/heston_book_reference.py) in long double, on the raw and on a centred basis: the restatements agree with
# each other to 1e-10 of a row and with the tape's VALUES to 1e-13, the tape's exposure-row gradients sit 4.3e-6 (American put) and
# 5.0e-5 (netting set) of a row away — the normal matrix of [1, S, S^2] has condition 1.5e12 there — and its PV rows 4e-15.  The
# forward pass with degree 2 is held to the float64 restatement on the GPU (tests/test_tangent_heston_gpu.py).
REGRESSION_DEGREE = {"heston_american_qe_aad": 1, "heston_netting_euler_aad": 1, "heston_bermudan_highpsi_qe_aad": 1}

# name -> (builder, n_pre, n_main, num_steps, scheme name)
CASES = {
    "heston_american_qe_aad": (american, 512, 512, 2, "QE"),
    "heston_netting_euler_aad": (netting, 512, 512, 4, "EULER"),
    "heston_bermudan_highpsi_qe_aad": (bermudan_highpsi, 512, 512, 2, "QE"),
}


def fixture_names():
    """the cases whose fixture is committed (the generator keeps a case only when its draws meet the margin condition)"""
    import os
    import cases
    return [k for k in CASES if os.path.exists(os.path.join(cases.GOLDEN, k + ".npz"))]


def injected_draws(g, backend=None):
    """{"pre" / "main": (z [S][2][N], u [S][N] or None)} from a fixture's recorded draws, numpy or on `backend`"""
    put = (lambda a: a) if backend is None else backend.from_numpy
    out = {}
    for which in ("pre", "main"):
        if f"z_{which}" not in g.files:
            continue
        z = put(np.ascontiguousarray(np.transpose(g[f"z_{which}"], (0, 2, 1))))
        u = put(np.ascontiguousarray(g[f"u_{which}"][:, :, 0])) if f"u_{which}" in g.files else None
        out[which] = (z, u)
    return out


def make_controller(name, backend, inject=True, tangent_heston=False, g=None, differentiate=True, degree=None):
    """the controller of `name`; with inject, on the draws the reference consumed (g: the fixture, loaded when None).  degree: of the
    regression polynomial instead of the case's own (REGRESSION_DEGREE)"""
    import cases
    build, n_pre, n_main, steps, scheme = CASES[name]
    ns, model, rm = build()
    degree = REGRESSION_DEGREE.get(name) if degree is None else degree
    kw = {"regression_function": cases.PolyomialRegression(degree=degree)} if degree is not None else {}
    sc = cases.SimulationController(ns, model, rm, n_main, n_pre, steps, getattr(cases.SimulationScheme, scheme), differentiate=differentiate,
                                    backend=backend, **kw)
    sc.materialize = True
    sc.tangent_heston = tangent_heston
    if inject:
        g = cases.load_golden(name) if g is None else g
        sc._inject.update(injected_draws(g, backend))
    return sc, g


def bare_tables(model, plan, smoothing):
    """(d0, dd) of aad.descriptor_tangents for a simulation without a book: the tables of a dual path kernel and their tangents [...][P]"""
    from mcx import aad
    bare = types.SimpleNamespace(sim_plan=plan, _comp=types.SimpleNamespace(atoms=[], atom_src=[]))
    return aad.descriptor_tangents(bare, model, smoothing, mode="complex")


def fixture_margins(name, g):
    """the margins of a fixture's draws (tests/heston_tangent_reference.py), pre-simulation and main: {which: margins}"""
    import cases
    import heston_tangent_reference as hr
    from mcx.plan import SimPlan
    build, n_pre, n_main, steps, scheme = CASES[name]
    ns, model, rm = build()
    model.perform_smoothing = True                                             # differentiate=True switches the smoothing on
    sc = cases.SimulationController(ns, model, rm, n_main, n_pre, steps, getattr(cases.SimulationScheme, scheme), differentiate=False,
                                    backend=types.SimpleNamespace(name="stub"))
    plan = SimPlan(model, sc.simulation_timeline.numpy(), sc.simulation_scheme, steps)
    tb = hr.tables_of(plan, *bare_tables(model, plan, True), True)
    return {which: hr.dual_paths(tb, z, u)[2] for which, (z, u) in injected_draws(g).items()}
