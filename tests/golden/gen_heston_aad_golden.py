#!/usr/bin/env python3
"""tests/golden/heston_*_aad.npz: the reference's results and autograd gradients of the Heston books of tests/heston_aad_cases.py (an
American put under QE, a two-option netting set under EULER, the American put with high-psi parameters), with differentiate=True.
Run where the reference is importable (as gen_golden.py, whose recorder and `run_controller_case` are reused):
    python tests/golden/gen_heston_aad_golden.py
Every fixture keeps its draws (injected normals, the QE uniforms), results, gradients and names, nothing per path.

Before a fixture is kept, the numpy restatement of the dual step maps (tests/heston_tangent_reference.py) runs on the fixture's own
draws, pre-simulation and main: no path value may be non-finite, and every margin — psi - 1.5 and u - p from the edges of their fuzzy
bands, the Euler variance from its floor, psi + eps from zero, the remaining clamps of the QE step from their kinks — must exceed
1e-9.  A path that close could take another mask on a device whose exp / log differ from torch's by ulps.  A case that violates the
condition gets another seed, at most 20 of them; a case that finds none is not kept and says so.  The reference's engines seed
torch themselves (42 for the pre-simulation, 43 for the main one): attempt k shifts both seeds by 100 k while the reference runs.

rho under EULER.  The reference's HestonModel stacks [[1, rho], [rho, 1]] in its constructor, BEFORE the controller marks the
parameters (Model.requires_grad): the matrix is a constant of the tape and d / d rho comes back as None under EULER, although rho
moves every correlated variance draw.  `_rho_on_tape` marks the parameters first and stacks the matrix again from the marked rho, so
that the tape goes through torch.linalg.cholesky of it — the derivative the project's kernels (kt_heston, kt_paths_heston) and a bump
of rho compute.  Nothing else of the reference is touched; under QE the matrix is not read."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "montecarlo-risk-engine_amd"))

import numpy as np
import torch

import gen_golden as ref                 # puts the reference on sys.path; `ref` is the namespace of its classes
import heston_aad_cases as hcases
import heston_tangent_reference as hr

MAX_SEEDS = 20
KEEP = ("z_", "u_", "result_", "grad_")


def _rho_on_tape(build):
    def wrapped():
        ns, model, rm = build(lib=ref)
        model.requires_grad()
        rho = model.get_rho().squeeze()
        one = torch.tensor(1.0, dtype=rho.dtype)
        model.correlation_matrix = torch.stack([torch.stack([one, rho]), torch.stack([rho, one])])
        return ns, model, rm
    return wrapped


def _run_reference(name, build, n_pre, n_main, steps, scheme, degree, shift):
    """one run of the reference under the recorder with the engines' seeds shifted by `shift`; -> the recorded npz as a dict, or None
    when the reference's lstsq stops on NaN paths (the smoothed QE step below a negative variance) — any other failure is raised"""
    own_seed = torch.manual_seed
    torch.manual_seed = lambda s: own_seed(int(s) + shift)
    try:
        ref.run_controller_case(name, _rho_on_tape(build), n_pre, n_main, steps, getattr(ref.SimulationScheme, scheme), differentiate=True,
                                degree=degree)
    except RuntimeError as e:
        if "torch.linalg.lstsq" not in str(e):
            raise
        return None
    finally:
        torch.manual_seed = own_seed
    g = np.load(os.path.join(HERE, name + ".npz"))
    return {k: g[k] for k in g.files}


def main():
    torch.set_num_threads(4)
    for name, (build, n_pre, n_main, steps, scheme) in hcases.CASES.items():
        path = os.path.join(HERE, name + ".npz")
        kept = False
        for seed in range(MAX_SEEDS):
            g = _run_reference(name, build, n_pre, n_main, steps, scheme, hcases.REGRESSION_DEGREE.get(name), 100 * seed)
            if g is None:
                print(f"{name} attempt {seed}: the reference's lstsq stopped on NaN paths; rejected")
                continue
            keep = {k: v for k, v in g.items() if k.startswith(KEEP) or k in ("param_names", "metric_names", "netting_set_names")}
            # the tape of these fixtures is not the unmodified reference's under EULER: see "rho under EULER" above
            keep["patched_rho"] = np.array(True)
            finite = bool(np.isfinite(g["paths_main"]).all() and ("paths_pre" not in g or np.isfinite(g["paths_pre"]).all()))
            np.savez_compressed(path, **keep)
            margins = hcases.fixture_margins(name, np.load(path))
            ok = finite and all(hr.margins_hold(m) for m in margins.values())
            print(f"{name} attempt {seed}: reference paths finite {finite}; margins {margins}; {'kept' if ok else 'rejected'}")
            if ok:
                # the same draws through the controller's default quadratic regression: results and gradients only (deg2_*), what
                # tests/test_tangent_heston_host.py holds against the host restatement in long double to place the tape's own error
                g2 = _run_reference(name, build, n_pre, n_main, steps, scheme, 2, 100 * seed)
                assert all(np.array_equal(g2[k], keep[k]) for k in keep if k.startswith(("z_", "u_")))
                keep.update({"deg2_" + k: v for k, v in g2.items() if k.startswith(("result_", "grad_"))})
                np.savez_compressed(path, **keep)
                kept = True
                print(f"{name}: kept draws, results and gradients, {os.path.getsize(path) / 1024:.0f} KiB")
                break
        if not kept:
            if os.path.exists(path):
                os.remove(path)
            print(f"{name}: no seed of {MAX_SEEDS} meets the margin condition; the case has no fixture")


if __name__ == "__main__":
    main()
