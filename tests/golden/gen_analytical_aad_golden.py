#!/usr/bin/env python3
"""tests/golden/{netting,bond_option,flexicall,basket3_multi}_aad.npz: the reference's results and autograd gradients of four books
under the ANALYTICAL scheme with differentiate=True (tests/analytical_aad_cases.py).  Run where the reference is importable (as
gen_golden.py, whose recorder, `run_controller_case` and `slim_to_gradients` are reused):
    python tests/golden/gen_analytical_aad_golden.py
The first three are cases of gen_golden.py: the engines seed torch themselves, so the draws are those of the base fixture
(netting.npz, bond_option.npz, flexicall.npz) — checked here bit for bit, the metric values to 1e-12, before the new fixture is
slimmed to results, gradients and names.  basket3_multi_aad keeps its own draws and drops the per-path dumps nobody reads (paths,
cashflows, exposures)."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import gen_golden as ref                 # puts the reference on sys.path; `ref` is the namespace of its classes
import analytical_aad_cases as aad_cases

SLIM = {"netting_aad": ref.case_netting, "bond_option_aad": ref.case_bond_option, "flexicall_aad": ref.case_flexicall}


def main():
    torch.set_num_threads(4)
    A = ref.SimulationScheme.ANALYTICAL
    for name, build in SLIM.items():
        _, n_pre, n_main, steps, base = aad_cases.CASES[name]
        ref.run_controller_case(name, build, n_pre, n_main, steps, A, differentiate=True)
        new, old = np.load(os.path.join(HERE, name + ".npz")), np.load(os.path.join(HERE, base + ".npz"))
        for key in [k for k in old.files if k.startswith(("z_", "u_"))]:
            assert new[key].tobytes() == old[key].tobytes(), (name, key)
        for key in [k for k in old.files if k.startswith("result_")]:      # (the regression's LAPACK solve moves the last bits run to run)
            assert np.allclose(new[key][:, 0], old[key][:, 0], rtol=1e-12, atol=1e-15), (name, key)
        ref.slim_to_gradients(name)
    name = "basket3_multi_aad"
    _, n_pre, n_main, steps, _ = aad_cases.CASES[name]
    ref.run_controller_case(name, lambda: aad_cases.basket3_multi(lib=ref), n_pre, n_main, steps, A, differentiate=True)
    path = os.path.join(HERE, name + ".npz")
    g = np.load(path)
    keep = {k: g[k] for k in g.files if k.startswith(("z_", "result_", "grad_")) or k in ("param_names", "metric_names", "netting_set_names")}
    np.savez_compressed(path, **keep)
    print(f"{name}: kept draws, results and gradients, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
