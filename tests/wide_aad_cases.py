"""Sensitivity cases of wide models whose fixtures hold the reference's autograd gradients (tests/golden/gen_wide_aad_golden.py builds
the same cases with the reference's classes: every builder takes the classes from `mod`).

wide_cva10_aad: the book of wide_cases.cva10 — one Vasicek short rate and nine CIR++ hazard models, one per counterparty, under a full
10 x 10 correlation matrix; three netting sets (a payer swap and a bond each) with three different counterparties; PV, EPE and one
CVAMetric per counterparty — with y0 = theta for every CIR++ model.  wide_cases.cva10 starts at y0 = 1e-4 (1 + k), where Euler paths
reach the 1e-12 floor: a tape and a dual kernel need not agree at that kink.  EULER, 2 sub-steps, 128 + 128 paths; the fixture holds
the draws the reference consumed, its metric values and its gradients, and the seed the generator kept."""
import os

import numpy as np

import wide_cases as wc

GOLDEN = wc.GOLDEN
FLOOR_DISTANCE = 1e-9          # the generator refuses draws that put a CIR++ path this close to its floor (or to 0)


def cva10_theta(mod: dict):
    ir = mod["VasicekModel"](0.0, 0.03, 0.05, 0.1, 0.01, asset_id="rates")
    cr = [mod["CIRPPModel"](0.0, f"cp{k}", wc.HAZARDS, kappa=0.1 + 0.02 * k, theta=0.01 + 0.001 * k, volatility=0.02 + 0.001 * k,
                            y0=0.01 + 0.001 * k) for k in range(9)]
    model = mod["ModelConfig"]([ir] + cr, inter_asset_correlation_matrix=wc.pair_blocks(wc.correlation(10, 32)))
    ns = []
    for j, k in enumerate(wc.CVA_COUNTERPARTIES):
        swap = mod["InterestRateSwap"](0.0, 1.0, 1.0 + 0.5 * j, 0.03 + 0.002 * j, 0.5, 0.5, mod["IRSType"].PAYER, "rates")
        swap.name = f"swap{j}"
        bond = mod["Bond"](0.0, 1.0, 0.5 + 0.25 * j, 0.5, True, 0.02 + 0.005 * j, "rates")
        bond.name = f"bond{j}"
        ns.append(mod["NettingSet"](name=f"ns{j}", products=[swap, bond], counterparty_id=f"cp{k}"))
    mets = [mod["PVMetric"](), mod["EPEMetric"]()] + [mod["CVAMetric"](f"cp{k}", 0.4) for k in wc.CVA_COUNTERPARTIES]
    return ns, model, mod["RiskMetrics"](mets, exposure_timeline=np.array([0.0, 0.5, 1.0]))


# name -> (builder, n_pre, n_main, num_steps, scheme name)
CASES = {"wide_cva10_aad": (cva10_theta, 128, 128, 2, "EULER")}


def load_golden(name: str):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def make_controller(name: str, backend, inject: bool = True, tangent_wide: bool = False, n_main: int | None = None,
                    n_pre: int | None = None):
    """the case with the mcx classes on `backend`, differentiate=True; inject: replay the reference's recorded draws"""
    from mcx.common.enums import SimulationScheme
    from mcx.controller.controller import SimulationController
    build, pre, main, steps, scheme = CASES[name]
    ns, model, rm = build(wc.mcx_classes())
    sc = SimulationController(ns, model, rm, main if n_main is None else n_main, pre if n_pre is None else n_pre, steps,
                              SimulationScheme[scheme], differentiate=True, backend=backend)
    sc.tangent_wide = tangent_wide
    g = load_golden(name)
    if inject:
        for key, where in (("z_main", "main"), ("z_pre", "pre")):
            sc._inject[where] = (backend.from_numpy(np.ascontiguousarray(np.transpose(g[key], (0, 2, 1)))), None)
    return sc, g
