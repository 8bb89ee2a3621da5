#!/usr/bin/env python3
"""Golden vectors of the wide sensitivity cases (tests/wide_aad_cases.py), by importing the Python reference like gen_wide_golden.py.

Run where the reference is installed:   python tests/golden/gen_wide_aad_golden.py
Writes wide_cva10_aad.npz: the draws the reference consumed (z_pre, z_main), its metric values and its autograd gradients, and `seed`.

The reference's tape and a dual kernel need not agree where a CIR++ path sits on the kink of its floor (max(y, 1e-12)) or of its root
(sqrt(max(y, 0))).  The generator therefore replays the recorded draws through the numpy restatement of the sub-steps
(tests/wide_paths_reference.py, on the plan the mcx classes build for the same case), takes the smallest CIR++ state BEFORE the
floor over every sub-step of both simulations, and refuses draws that bring one within FLOOR_DISTANCE = 1e-9 of the floor: it then
tries the next seed.  The seed it kept is recorded in the fixture."""
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
import gen_wide_golden as gw
import wide_aad_cases as wa
import wide_paths_reference as wr

KEEP = ("grad_", "param_names", "result_", "metric_names", "netting_set_names", "z_pre", "z_main", "simulation_timeline")
FIRST_SEED, MAX_TRIES = 20261021, 16


def smallest_cir_state(build, steps, scheme, timeline, z_blocks) -> float:
    """the smallest CIR++ state before the floor over every sub-step of the recorded simulations, in long double"""
    # (the mcx package keeps its modules named like the reference's — models, products, ... — inside its own namespace)
    sys.path.append(os.path.join(os.path.dirname(TESTS), "montecarlo-risk-engine_amd"))
    import wide_cases as wc
    from mcx.common.enums import SimulationScheme
    from mcx.plan import SimPlan
    _ns, model, _rm = build(wc.mcx_classes())
    plan = SimPlan(model, np.asarray(timeline, dtype=np.float64), SimulationScheme[scheme], steps)
    return min(wr.run(plan, np.ascontiguousarray(np.transpose(z, (0, 2, 1))), wr.LD).min_y for z in z_blocks)


def main():
    for name, (build, n_pre, n_main, steps, scheme) in wa.CASES.items():
        path = os.path.join(HERE, name + ".npz")
        for seed in range(FIRST_SEED, FIRST_SEED + MAX_TRIES):
            torch.manual_seed(seed)
            # The CVA of ANOTHER counterparty's netting set is a constant zero that never touched the tape, and torch.autograd.grad
            # raises on such an output.  Its gradient is recorded as unused (None -> NaN in the fixture), which
            # check_lsm_sensitivities reads as "must come back as zero".
            grad = torch.autograd.grad
            torch.autograd.grad = lambda out, inputs, **kw: grad(out, inputs, **kw) if out.requires_grad else tuple(None for _ in inputs)
            try:
                gg.run_controller_case(name, lambda: build(gw.REF_CLASSES), n_pre, n_main, steps, gg.SimulationScheme[scheme],
                                       differentiate=True)
            finally:
                torch.autograd.grad = grad
            g = np.load(path)
            low = smallest_cir_state(build, steps, scheme, g["simulation_timeline"], [g["z_pre"], g["z_main"]])
            if low - wr.FLOOR > wa.FLOOR_DISTANCE:
                break
            print(f"{name}: seed {seed} refused, a CIR++ path comes within {low - wr.FLOOR:.3e} of its floor")
        else:
            os.remove(path)
            raise SystemExit(f"{name}: no seed of {MAX_TRIES} keeps the CIR++ paths off their floor")
        np.savez_compressed(path, seed=np.int64(seed), smallest_cir_state=np.float64(low),
                            **{k: g[k] for k in g.files if k.startswith(KEEP)})
        print(name, "seed", seed, "smallest CIR++ state", low, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
