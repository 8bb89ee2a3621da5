"""Sensitivities under the ANALYTICAL scheme: the cases behind tests/golden/{netting,bond_option,flexicall,basket3_multi}_aad.npz
(recorded from the reference by tests/golden/gen_analytical_aad_golden.py) and american_put_aad.npz.  Three of them are builders of
tests/cases.py run with differentiate=True — their fixtures hold results and gradients only, the draws are the base fixture's —,
`basket3_multi` is a case of its own with its own draws.  `lib` is the namespace the classes are taken from: tests/cases.py (mcx) by
default, the reference's own classes when the generator records the fixtures."""
import numpy as np


def basket3_multi(lib=None):
    """three correlated assets in a BlackScholesMulti (odd number of normals, full lower-triangular factor), two arithmetic baskets
    without control variate in two netting sets, PV and EPE on [0, .3, .75, 1]"""
    if lib is None:
        import cases as lib
    ids = ["a1", "a2", "a3"]
    model = lib.BlackScholesMulti(0.0, 0.02, ids, [100, 105, 95], [0.4, 0.3, 0.25], [[1, .5, -.2], [.5, 1, .3], [-.2, .3, 1]])
    call = lib.BasketOption(1.0, ids, [.5, .3, .2], 100, lib.OptionType.CALL, lib.BasketOptionType.ARITHMETIC, False); call.name = "basket_call"
    put = lib.BasketOption(1.0, ids, [.25, .25, .5], 102, lib.OptionType.PUT, lib.BasketOptionType.ARITHMETIC, False); put.name = "basket_put"
    ns = [lib.NettingSet(name="call_set", products=[call]), lib.NettingSet(name="put_set", products=[put])]
    return ns, model, lib.RiskMetrics([lib.PVMetric(), lib.EPEMetric()], exposure_timeline=np.array([0.0, 0.3, 0.75, 1.0]))


# name -> (builder: a name of tests/cases.py or a function here, n_pre, n_main, num_steps, fixture that holds the draws)
CASES = {
    "american_put_aad": ("american", 2048, 1024, 1, "american_put"),
    "netting_aad": ("netting", 1024, 1024, 1, "netting"),
    "bond_option_aad": ("bond_option", 0, 1024, 2, "bond_option"),
    "flexicall_aad": ("flexicall", 2048, 1024, 1, "flexicall"),
    "basket3_multi_aad": (basket3_multi, 512, 512, 2, "basket3_multi_aad"),
}


def build(name):
    import cases
    builder = CASES[name][0]
    return builder() if callable(builder) else getattr(cases, builder)()


def make_controller(name, backend, inject=True, n_pre=None, n_main=None):
    """the differentiate=True controller of `name` under ANALYTICAL; with inject, on the draws the reference consumed"""
    import cases
    _, pre, main, steps, draws = CASES[name]
    ns, model, rm = build(name)
    sc = cases.SimulationController(ns, model, rm, main if n_main is None else n_main, pre if n_pre is None else n_pre, steps, cases.A,
                                    differentiate=True, backend=backend)
    sc.materialize = True
    g = cases.load_golden(name)
    if inject:
        gd = cases.load_golden(draws)
        for key, which in (("z_main", "main"), ("z_pre", "pre")):
            if key in gd.files:
                sc._inject[which] = (backend.from_numpy(np.ascontiguousarray(np.transpose(gd[key], (0, 2, 1)))), None)      # [S][n_z][N]
    return sc, g
