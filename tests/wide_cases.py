"""Wide models (more than MCX_MAX_SLOTS = 8 correlated one-factor sub-models): the models of the kernel-level tests and the
controller cases behind tests/golden/wide_*.npz (tests/golden/gen_wide_golden.py builds the same cases with the reference's
classes: every builder takes the classes from `mod`).

Shapes of the kernel-level tests: the timeline TIMELINE holds the calibration date (one stored date without a step) and two
distinct gaps, with NUM_STEPS = 2 sub-steps per gap, hence two distinct dt (two covariance factors under ANALYTICAL); path
counts N_PATHS = 1 / 255 / 257 (one lane, a block less one lane, a block and a lane) in a tensor whose leading dimension is
padded by LD_PAD doubles."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TIMELINE = np.array([0.0, 0.25, 0.6])
NUM_STEPS = 2
N_PATHS = (1, 255, 257)
LD_PAD = 7

HAZARDS = {
    0.5: 0.006402303360855854, 1.0: 0.01553038972325307, 2.0: 0.009729741230773657,
    3.0: 0.015552544648116201, 4.0: 0.021196186202801115, 5.0: 0.02284319986706472,
    7.0: 0.010111423894480876, 10.0: 0.00613267811172937, 15.0: 0.0036969930706003337,
    20.0: 0.003791311459217732,
}


def correlation(n: int, seed: int) -> np.ndarray:
    """a full n x n correlation matrix, no entry zero, smallest eigenvalue >= 0.3: three common factors plus idiosyncratic weight"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, size=(n, 3))
    c = 0.6 * (a @ a.T) / 3.0
    c = c + np.diag(1.0 - np.diag(c))
    d = np.sqrt(np.diag(c))
    c = c / np.outer(d, d)
    c = 0.7 * c + 0.3 * np.eye(n)
    return 0.5 * (c + c.T)


def pair_blocks(corr: np.ndarray) -> list:
    """ModelConfig's inter-asset argument for one-asset sub-models: a 1 x 1 block per model pair (i < j), in that order"""
    n = corr.shape[0]
    return [np.array([[corr[i, j]]]) for i in range(n) for j in range(i + 1, n)]


def mcx_classes() -> dict:
    from mcx.metrics.cva_metric import CVAMetric
    from mcx.metrics.epe_metric import EPEMetric
    from mcx.metrics.pfe_metric import PFEMetric
    from mcx.metrics.pv_metric import PVMetric
    from mcx.metrics.risk_metrics import RiskMetrics
    from mcx.models.black_scholes import BlackScholesModel
    from mcx.models.black_scholes_multi import BlackScholesMulti
    from mcx.models.cirpp import CIRPPModel
    from mcx.models.hull_white import HullWhiteModel
    from mcx.models.model_config import ModelConfig
    from mcx.models.vasicek import VasicekModel
    from mcx.products.basket_option import BasketOption, BasketOptionType
    from mcx.products.bond import Bond
    from mcx.products.equity import Equity
    from mcx.products.european_option import EuropeanOption
    from mcx.products.netting_set import NettingSet
    from mcx.products.product import OptionType
    from mcx.products.swap import InterestRateSwap, IRSType
    return dict(locals())


# ---- models of the kernel-level tests ------------------------------------------------------------------------------------------------
# slot kinds by letter: B Black-Scholes, V Vasicek, H Hull-White, C CIR++, D deterministic CIR++
def slot_model(letter: str, k: int, mod: dict):
    """sub-model k of a mix; parameters vary with k.  CIR++: y0 = theta = 0.03 .. 0.05 with a volatility far inside the Feller bound,
    so that no path comes near the 1e-12 floor on TIMELINE (tests assert it)"""
    if letter == "B":
        return mod["BlackScholesModel"](0.0, 80.0 + 7.0 * k, 0.01 + 0.002 * k, 0.15 + 0.02 * (k % 9), asset_id=f"eq{k}")
    if letter == "V":
        return mod["VasicekModel"](0.0, 0.02 + 0.001 * k, 0.03 + 0.002 * k, 0.2 + 0.05 * k, 0.008 + 0.0005 * k, asset_id=f"ir{k}")
    if letter == "H":
        ts = np.linspace(0.0, 25.0, 26)
        f = 0.03 + 0.02 * np.sin(ts / (3.0 + 0.25 * k)) + 0.001 * k
        return mod["HullWhiteModel"](0.0, float(f[0]), list(f), list(np.gradient(f, ts)), 0.1 + 0.03 * k, 0.01 + 0.0004 * k,
                                     asset_id=f"hw{k}", curve_times=list(ts))
    if letter in "CD":
        lvl = 0.03 + 0.0007 * k
        return mod["CIRPPModel"](0.0, f"cp{k}", HAZARDS, kappa=0.4 + 0.02 * k, theta=lvl, volatility=0.04 + 0.001 * (k % 7), y0=lvl,
                                 deterministic=letter == "D")
    raise ValueError(letter)


def mixed_model(letters: str, seed: int, mod: dict | None = None):
    """ModelConfig of len(letters) one-factor sub-models under a full correlation matrix"""
    mod = mod or mcx_classes()
    models = [slot_model(c, k, mod) for k, c in enumerate(letters)]
    if len(models) == 1:
        return models[0]
    return mod["ModelConfig"](models, inter_asset_correlation_matrix=pair_blocks(correlation(len(models), seed)))


def bs_multi(n: int, seed: int, mod: dict | None = None):
    mod = mod or mcx_classes()
    ids = [f"asset{k}" for k in range(n)]
    return mod["BlackScholesMulti"](0.0, 0.02, ids, [90.0 + 3.0 * k for k in range(n)], [0.15 + 0.01 * (k % 11) for k in range(n)],
                                    correlation(n, seed))


def _mix(n: int) -> str:
    """n slots cycling through all five kinds, starting with a Vasicek numeraire"""
    return "".join("VBCHD"[k % 5] for k in range(n))


# name -> (builder of the model, scheme name): what the narrow route can also run (equality) ...
NARROW = {
    "vas_cir_2_euler": (lambda: mixed_model("VC", 11), "EULER"),
    "mix_5_euler": (lambda: mixed_model("BBVCD", 12), "EULER"),
    "mix_8_euler": (lambda: mixed_model("BBBBVHCC", 13), "EULER"),
    "bs_4_analytical": (lambda: bs_multi(4, 14), "ANALYTICAL"),
    "vas_1_analytical": (lambda: mixed_model("V", 15), "ANALYTICAL"),
}
# ... and what it cannot
WIDE = {
    "mix_9_euler": (lambda: mixed_model(_mix(9), 21), "EULER"),
    "mix_16_euler": (lambda: mixed_model(_mix(16), 22), "EULER"),
    "mix_17_euler": (lambda: mixed_model(_mix(17), 23), "EULER"),
    "mix_32_euler": (lambda: mixed_model(_mix(32), 24), "EULER"),
    "bs_12_analytical": (lambda: bs_multi(12, 25), "ANALYTICAL"),
    "bs_32_analytical": (lambda: bs_multi(32, 26), "ANALYTICAL"),
}


def plan_of(name: str, force_wide: bool = False):
    from mcx.common.enums import SimulationScheme
    from mcx.plan import SimPlan
    build, scheme = (NARROW.get(name) or WIDE[name])
    return SimPlan(build(), TIMELINE, SimulationScheme[scheme], NUM_STEPS, force_wide=force_wide)


# ---- controller cases behind the fixtures --------------------------------------------------------------------------------------------
def basket12(mod: dict):
    """12-asset BlackScholesMulti: an arithmetic basket call without control variate and a European call on asset 11, in one
    netting set; PV, EPE and PFE(0.95) on 3 dates"""
    n = 12
    ids = [f"asset{k}" for k in range(n)]
    model = mod["BlackScholesMulti"](0.0, 0.02, ids, [95.0 + 2.0 * k for k in range(n)], [0.18 + 0.015 * k for k in range(n)],
                                     correlation(n, 31))
    w = np.arange(1.0, n + 1.0)
    basket = mod["BasketOption"](1.0, ids, list(w / w.sum()), 105.0, mod["OptionType"].CALL, mod["BasketOptionType"].ARITHMETIC, False)
    basket.name = "basket12"
    euro = mod["EuropeanOption"](mod["Equity"](ids[11]), 1.0, 115.0, mod["OptionType"].CALL, asset_id=ids[11])
    euro.name = "call_asset11"
    ns = [mod["NettingSet"](name="book", products=[basket, euro])]
    rm = mod["RiskMetrics"]([mod["PVMetric"](), mod["EPEMetric"](), mod["PFEMetric"](0.95)], exposure_timeline=np.array([0.0, 0.5, 1.0]))
    return ns, model, rm


CVA_COUNTERPARTIES = (0, 3, 8)


def cva10(mod: dict):
    """one Vasicek short rate and nine CIR++ hazard models (one per counterparty) under a full 10 x 10 correlation matrix; three
    netting sets with three different counterparties, each a payer swap and a bond (semi-annual, one year: three simulated dates keep the fixture small); PV, EPE and one CVAMetric per
    counterparty"""
    ir = mod["VasicekModel"](0.0, 0.03, 0.05, 0.1, 0.01, asset_id="rates")
    cr = [mod["CIRPPModel"](0.0, f"cp{k}", HAZARDS, kappa=0.1 + 0.02 * k, theta=0.01 + 0.001 * k, volatility=0.02 + 0.001 * k,
                            y0=1e-4 * (1 + k)) for k in range(9)]
    model = mod["ModelConfig"]([ir] + cr, inter_asset_correlation_matrix=pair_blocks(correlation(10, 32)))
    ns = []
    for j, k in enumerate(CVA_COUNTERPARTIES):
        swap = mod["InterestRateSwap"](0.0, 1.0, 1.0 + 0.5 * j, 0.03 + 0.002 * j, 0.5, 0.5, mod["IRSType"].PAYER, "rates")
        swap.name = f"swap{j}"
        bond = mod["Bond"](0.0, 1.0, 0.5 + 0.25 * j, 0.5, True, 0.02 + 0.005 * j, "rates")
        bond.name = f"bond{j}"
        ns.append(mod["NettingSet"](name=f"ns{j}", products=[swap, bond], counterparty_id=f"cp{k}"))
    mets = [mod["PVMetric"](), mod["EPEMetric"]()] + [mod["CVAMetric"](f"cp{k}", 0.4) for k in CVA_COUNTERPARTIES]
    return ns, model, mod["RiskMetrics"](mets, exposure_timeline=np.array([0.0, 0.5, 1.0]))


# name -> (builder, n_pre, n_main, num_steps, scheme name, differentiate, fixture holding the draws)
CASES = {
    "wide_basket12_analytical": (basket12, 128, 128, 1, "ANALYTICAL", False, None),
    "wide_basket12_euler": (basket12, 128, 128, 1, "EULER", False, None),
    "wide_cva10": (cva10, 128, 128, 2, "EULER", False, None),
    # sensitivities by bump-and-revalue against the reference's autograd: gradients only, draws = the base case's
    "wide_basket12_analytical_aad": (basket12, 128, 128, 1, "ANALYTICAL", True, "wide_basket12_analytical"),
}


def load_golden(name: str):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def make_controller(name: str, backend, inject: bool = True, fused: bool = True, n_main: int | None = None, n_pre: int | None = None):
    """the case with the mcx classes on `backend`; inject: replay the reference's recorded draws"""
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    build, pre, main, steps, scheme, diff, draws = CASES[name]
    ns, model, rm = build(mcx_classes())
    sc = SimulationController(ns, model, rm, main if n_main is None else n_main, pre if n_pre is None else n_pre, steps,
                              SimulationScheme[scheme], differentiate=diff, backend=backend)
    sc.materialize = True
    sc.allow_fused = fused
    g = load_golden(name) if inject or diff else None
    if inject:
        gd = load_golden(draws or name)
        for key, where in (("z_main", "main"), ("z_pre", "pre")):
            sc._inject[where] = (backend.from_numpy(np.ascontiguousarray(np.transpose(gd[key], (0, 2, 1)))), None)
    return sc, g
