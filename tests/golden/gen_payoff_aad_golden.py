#!/usr/bin/env python3
"""tests/golden/payoff_*_aad.npz: the reference's results and autograd gradients of the payoff-form books of
tests/payoff_aad_cases.py (binary, barrier with and without Brownian bridge, control-variate and geometric basket, geometric Asian,
an exposure book through a pre-simulation), with differentiate=True.  Run where the reference is importable (as gen_golden.py,
whose recorder, `run_controller_case` and `_RecordingRng` are reused):
    python tests/golden/gen_payoff_aad_golden.py
Every fixture keeps its draws (injected normals, recorded bridge uniforms), results, gradients and names, nothing per path.

Before a fixture is kept, the numpy restatement of the dual forms (tests/payoff_tangent_reference.py) runs on the fixture's own draws
through the oracle backend's paths: no path's clamp argument may lie within 1e-9 (in band units) of a band edge, no payoff within
1e-9 of its kink, no two extremal monitored spots within 1e-9 (relative) of each other.  A path that close could take another mask
on a device whose exp / log differ from torch's by ulps.  A case that violates it gets another seed (SEEDS), not another condition."""
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
import payoff_aad_cases as pcases

MARGIN = 1e-9
SEEDS = {}                               # case -> torch seed set before the reference runs (default: the engines' own)


def _record_bridge(build):
    def wrapped():
        ns, model, rm = build(lib=ref)
        for n in ns:
            for p in n.products:
                if getattr(p, "use_brownian_bridge", False):
                    p.rng = ref._RecordingRng(p.rng)
        return ns, model, rm
    return wrapped


def _check_margins(name):
    """the condition of the module docstring, on the mcx book plan of the case and the oracle backend's paths of the fixture's draws"""
    from oracle_backend import OracleBackend
    from payoff_tangent_reference import PayoffRestatement
    sc, g = pcases.make_controller(name, OracleBackend(), differentiate=False)
    sc.run_simulation()
    worst = np.inf
    for key in ("paths", "paths_pre"):
        paths = sc.last_state.get(key)
        if paths is None:
            continue
        paths = np.asarray(paths)
        rs = PayoffRestatement(sc.book_plan, paths, np.zeros((1,) + paths.shape), np.zeros((len(sc.book_plan.atoms), 5, 1)), None,
                               pcases.bridge_rows(g) if key == "paths" else None)
        pr = sc.book_plan.products
        for p in range(len(pr)):
            for q in range(pr["cf_begin"][p], pr["cf_end"][p]):
                e = sc.book_plan.events[q]
                if key == "paths_pre" and e["aux"][0] == 5.0:
                    continue                                                   # (no bridge event in a pre-simulated case)
                rs.event(q)
        worst = min(worst, rs.smallest_margin())
    assert worst > MARGIN, (name, worst)
    return worst


def main():
    torch.set_num_threads(4)
    for name, (build, n_pre, n_main, steps, scheme) in pcases.CASES.items():
        if name in SEEDS:
            torch.manual_seed(SEEDS[name])
        ref.run_controller_case(name, _record_bridge(build), n_pre, n_main, steps, getattr(ref.SimulationScheme, scheme), differentiate=True,
                                extra=ref._bridge_extra)
        path = os.path.join(HERE, name + ".npz")
        g = np.load(path)
        keep = {k: g[k] for k in g.files if k.startswith(("z_", "bridge_u_", "result_", "grad_")) or k in ("param_names", "metric_names", "netting_set_names")}
        np.savez_compressed(path, **keep)
        worst = _check_margins(name)
        print(f"{name}: kept draws, results and gradients, {os.path.getsize(path) / 1024:.0f} KiB; smallest margin {worst:.3e}")


if __name__ == "__main__":
    main()
