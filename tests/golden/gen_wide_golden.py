#!/usr/bin/env python3
"""Golden vectors of the wide-model cases (tests/wide_cases.py), by importing the Python reference like gen_golden.py: the draw
recorder and the controller runner are gen_golden's, the cases are built from wide_cases with the reference's classes.

Run where the reference is installed:   python tests/golden/gen_wide_golden.py
Writes wide_basket12_{analytical,euler}.npz, wide_cva10.npz (draws, paths, coefficients, cashflows, exposures, metric values) and
wide_basket12_analytical_aad.npz (the reference's autograd gradients only; its draws are the base case's)."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import gen_golden as gg          # puts the reference's src/ on sys.path and imports its classes
import wide_cases as wc

REF_CLASSES = {k: getattr(gg, k) for k in (
    "CVAMetric", "EPEMetric", "PFEMetric", "PVMetric", "RiskMetrics", "BlackScholesModel", "BlackScholesMulti", "CIRPPModel",
    "ModelConfig", "VasicekModel", "BasketOption", "BasketOptionType", "Bond", "Equity", "EuropeanOption", "NettingSet", "OptionType",
    "InterestRateSwap", "IRSType")}
KEEP_AAD = ("grad_", "param_names", "result_", "metric_names", "netting_set_names")


def main():
    for name, (build, n_pre, n_main, steps, scheme, diff, draws) in wc.CASES.items():
        torch.manual_seed(20261020 + len(draws or name))          # a gradient case repeats the draws of its base case
        gg.run_controller_case(name, lambda: build(REF_CLASSES), n_pre, n_main, steps, gg.SimulationScheme[scheme], differentiate=diff)
        path = os.path.join(HERE, name + ".npz")
        if draws is not None:
            g = np.load(path)
            base = np.load(os.path.join(HERE, draws + ".npz"))
            assert np.array_equal(g["z_main"], base["z_main"]) and np.array_equal(g["z_pre"], base["z_pre"]), "draws differ from the base case"
            np.savez_compressed(path, **{k: g[k] for k in g.files if k.startswith(KEEP_AAD)})
        print(name, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
