"""The reference's large-netting-set CVA workload (tests/exposure_tests/cva_large_netting_set_derivatives.py:57-167 there) restated
with the mcx classes: European calls + bonds + unequal-tenor payer swaps in one netting set, CVA under Black-Scholes + Vasicek +
deterministic CIR++ and EULER.  `lib` is the namespace the classes are taken from: tests/cases.py (mcx) by default, the reference's
own classes when tests/golden/gen_large_cva_aad_golden.py records the fixture."""
import numpy as np

COUNTERPARTY_ID = "large_counterparty"
FULL = dict(num_europeans=20, num_bonds=10, num_swaps=150, exposure_timeline=np.linspace(0.0, 6.0, 60), num_steps=4, n_pre=512, n_main=512)
# the committed fixture (tests/golden/large_cva_aad.npz): 72 products, above the 64 of the per-job route
SMALL = dict(num_europeans=8, num_bonds=4, num_swaps=60, exposure_timeline=np.linspace(0.0, 4.0, 12), num_steps=2, n_pre=256, n_main=256)


def build(num_europeans, num_bonds, num_swaps, exposure_timeline, spot=100.0, rate_level=0.03, sigma=0.22, lib=None):
    if lib is None:
        import cases as lib
    products = []
    maturities, strike_scales = np.linspace(0.5, 3.0, 8), np.linspace(0.85, 1.15, 10)
    for idx in range(num_europeans):
        o = lib.EuropeanOption(lib.Equity("equity"), float(maturities[idx % 8]), 100.0 * float(strike_scales[idx % 10]),
                               lib.OptionType.CALL, asset_id="equity")
        o.name = f"large_european_call_{idx}"
        products.append(o)
    maturities, coupons = np.linspace(2.0, 6.0, 8), np.linspace(0.018, 0.030, 5)
    for idx in range(num_bonds):
        b = lib.Bond(0.0, float(maturities[idx % 8]), 2.0, 0.5, True, float(coupons[idx % 5]), "rates")
        b.name = f"large_bond_{idx}"
        products.append(b)
    maturities, fixed = np.linspace(2.0, 6.0, 8), np.linspace(0.019, 0.031, 6)
    for idx in range(num_swaps):
        s = lib.InterestRateSwap(0.0, float(maturities[idx % 8]), 25.0, float(fixed[idx % 6]), 0.5, 0.25, lib.IRSType.PAYER, "rates")
        s.name = f"large_swap_{idx}"
        products.append(s)
    ns = [lib.NettingSet(name="large_cva_ns", products=products, counterparty_id=COUNTERPARTY_ID)]
    eq = lib.BlackScholesModel(0.0, spot, rate_level, sigma, asset_id="equity")
    ra = lib.VasicekModel(0.0, rate_level, 0.03, 1.0, 0.01, asset_id="rates")
    cr = lib.CIRPPModel(0.0, COUNTERPARTY_ID, lib.HAZARDS, kappa=0.10, theta=0.01, volatility=0.02, y0=1e-4, deterministic=True)
    model = lib.ModelConfig([eq, ra, cr], inter_asset_correlation_matrix=[np.array([0.0])] * 3)
    return ns, model, lib.RiskMetrics([lib.CVAMetric(COUNTERPARTY_ID, 0.4)], exposure_timeline=np.asarray(exposure_timeline))


def make_controller(backend, inject=True, cfg=SMALL, differentiate=True):
    """the controller of `cfg`; with inject, on the draws recorded in large_cva_aad.npz (cfg must be SMALL then)"""
    import cases
    ns, model, rm = build(cfg["num_europeans"], cfg["num_bonds"], cfg["num_swaps"], cfg["exposure_timeline"])
    sc = cases.SimulationController(ns, model, rm, cfg["n_main"], cfg["n_pre"], cfg["num_steps"], cases.E, differentiate=differentiate,
                                    backend=backend)
    sc.materialize = True
    g = None
    if inject:
        g = cases.load_golden("large_cva_aad")
        for key, which in (("z_main", "main"), ("z_pre", "pre")):
            sc._inject[which] = (backend.from_numpy(np.ascontiguousarray(np.transpose(g[key], (0, 2, 1)))), None)      # [S][n_z][N]
    return sc, g
