#!/usr/bin/env python3
"""Golden vectors of the FVA sensitivities, by IMPORTING the Python reference like gen_fva_golden.py.

Run where the reference is installed:   python tests/golden/gen_fva_aad_golden.py
The book and the metric are those of gen_fva_golden.py (RefFVA: a subclass of the reference's CVAMetric that evaluates the table of
mcx/metrics/fva_metric.py on the reference's own exposures and requests), here with differentiate=True: the reference's autograd
differentiates the three evaluations through pre-simulation, regression and main simulation.  The funding weights are plain floats:
they carry no gradient, as in mcx_tangent_fva.

Writes fva_irs_aad.npz: the draws the reference consumed (z_pre, z_main), its exposures, the three values and errors (result_0_0),
their gradients [3][12] (grad_0_0), the names, the metric timeline, the two spread curves and `seed`.

The draws are screened as gen_xva_aad_golden.py screens them: the recorded draws are replayed through the numpy restatement of the
sub-steps, and draws that bring a CIR++ state of either name within FLOOR_DISTANCE = 1e-9 of its floor are refused (the reference's
tape and a dual kernel need not agree on that kink); the generator then tries the next seed and records the one it kept."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)

import numpy as np
import torch

import gen_golden as gg          # puts the reference's src/ on sys.path and imports its classes
import gen_fva_golden as gf
import gen_xva_aad_golden as ga

NAME = "fva_irs_aad"


def build():
    """the book of gen_fva_golden.main, on the reference's classes"""
    ns, model, _rm = ga.build()
    rm = gf.RiskMetrics([gf.RefFVA(gf.BORROW_CURVE, gf.LEND_CURVE, "cp", "own")], exposure_timeline=np.arange(11) * 0.25)
    return ns, model, rm


def main():
    torch.set_num_threads(4)
    path = os.path.join(HERE, NAME + ".npz")
    for seed in range(ga.FIRST_SEED, ga.FIRST_SEED + ga.MAX_TRIES):
        manual_seed = torch.manual_seed
        torch.manual_seed = lambda s, _off=1000 * seed: manual_seed(s + _off)
        try:
            gg.run_controller_case(NAME, build, gf.N_PATHS, gf.N_PATHS, ga.STEPS, gg.SimulationScheme.EULER, differentiate=True)
        finally:
            torch.manual_seed = manual_seed
        g = np.load(path)
        low = ga.smallest_cir_state(g["simulation_timeline"], [g["z_pre"], g["z_main"]])
        if low - ga.wr.FLOOR > ga.FLOOR_DISTANCE:
            break
        print(f"{NAME}: seed {seed} (offset {1000 * seed}) refused, a CIR++ path comes within {low - ga.wr.FLOOR:.3e} of its floor")
    else:
        os.remove(path)
        raise SystemExit(f"{NAME}: no seed of {ga.MAX_TRIES} keeps the CIR++ paths off their floor")
    grad = g["grad_0_0"]
    names = list(g["param_names"])
    assert grad.shape == (3, len(names)) and np.isfinite(grad).all()
    np.savez_compressed(path, seed=np.int64(seed), smallest_cir_state=np.float64(low), evaluations=np.array(gf.EVALUATIONS),
                        borrow_tenors=np.array(list(gf.BORROW_CURVE.keys())), borrow_spreads=np.array(list(gf.BORROW_CURVE.values())),
                        lend_tenors=np.array(list(gf.LEND_CURVE.keys())), lend_spreads=np.array(list(gf.LEND_CURVE.values())),
                        **{k: g[k] for k in g.files if k.startswith(ga.KEEP)})
    print(NAME, "seed", seed, "smallest CIR++ state", low, os.path.getsize(path) // 1024, "KiB")
    print("parameters:", names)
    print("gradient [3][P]:\n", grad)


if __name__ == "__main__":
    main()
