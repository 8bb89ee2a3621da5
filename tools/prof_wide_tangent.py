"""Timings of the forward-mode route for wide models (csrc/kt_wide.hip, mcx.aad.wide_route).  Needs the GPU.

  --driver BOOK ROUTE   one process: run_simulation(differentiate=True) of BOOK at --paths + --paths Philox paths with tangent_wide =
                        (ROUTE == "wide"; "bump": the flag off), warmed by a 4,096-path run and one full-size run, then --reps timed
                        runs; prints one JSON line.  BOOK: basket12 (tests/wide_cases.py, 12-asset basket, ANALYTICAL, 25
                        parameters) or cva10 (tests/wide_aad_cases.py: the ten-factor CVA book with y0 = theta, EULER, 40 parameters).
                        Protocol of the README: fresh processes, the two routes interleaved, three repetitions — start this tool once
                        per (book, route, repetition) from a shell loop.
  --kernel CASE         one process: --reps calls of mcx_tangent_paths_wide on a 32-slot EULER model (Black-Scholes, Vasicek, CIR++
                        in turn), --paths paths x 100 sub-steps to one stored date, with the tables of CASE: last (slot 31 alone),
                        first2 (slots 0 and 1), all (every slot), and as many calls of mcx_generate_paths.  Run it under
                        `rocprofv3 --kernel-trace --stats -- python tools/prof_wide_tangent.py --kernel CASE` in a run of its own and
                        read the device time per launch of kt_paths_wide and of k1_paths_wide<32, false> from the stats.  The cost
                        model to check: sum over the active r of (r >> 1) + 1 Philox pairs per path-step against 16 of the primal."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "montecarlo-risk-engine_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

ACTIVE = {"last": [31], "first2": [0, 1], "all": list(range(32))}


def driver(book, route, paths, reps):
    import wide_aad_cases as wa
    import wide_cases as wc
    from mcx import _native
    hip = _native.HipBackend(0)

    def run(n):
        if book == "basket12":
            sc, _ = wc.make_controller("wide_basket12_analytical_aad", hip, inject=False, n_main=n, n_pre=n)
        else:
            sc, _ = wa.make_controller("wide_cva10_aad", hip, inject=False, n_main=n, n_pre=n)
        sc.materialize, sc.tangent_wide = False, route == "wide"
        t0 = time.perf_counter()
        sc.run_simulation()
        hip.synchronize()
        return time.perf_counter() - t0, sc.timings

    run(4096)
    run(paths)
    out = [run(paths) for _ in range(reps)]
    keep = ("tangent", "forward_mode_passes", "bumped_passes", "wide_active_slots")
    print(json.dumps(dict(book=book, route=route, paths=paths, seconds=[round(t, 4) for t, _ in out],
                          timings={k: out[-1][1][k] for k in keep if k in out[-1][1]})), flush=True)


def kernel(case, reps, paths, steps=100):
    import wide_cases as wc
    from mcx import _abi, _native
    from mcx.common.enums import SimulationScheme
    from mcx.plan import SimPlan
    hip = _native.HipBackend(0)
    model = wc.mixed_model("".join("BVC"[k % 3] for k in range(32)), 24)
    plan = SimPlan(model, np.array([1.0]), SimulationScheme.EULER, steps)
    sim = plan.create_sim(hip)
    NP = _abi.TANGENT_NP
    dslot, dinit = np.zeros((32, _abi.SLOT_NPARAM, NP)), np.zeros((plan.n_state, NP))
    daux = np.zeros((plan.n_steps, 32, _abi.AUX, NP))
    for r in ACTIVE[case]:
        dslot[r, 1, r % NP] = 1.0                       # d sigma of slot r = direction r mod NP
    out = (hip.empty(plan.n_dates, plan.n_state, paths), hip.empty(NP, plan.n_dates, plan.n_state, paths))
    n_active = -1
    for _ in range(reps + 2):
        n_active = hip.tangent_paths_wide(sim, dslot, dinit, daux, None, 43, 0, paths, out=out)[2]
        hip.generate_paths(sim, 43, 0, paths, out=out[0])
        hip.synchronize()
    print(json.dumps(dict(case=case, paths=paths, sub_steps=steps, n_active=n_active, launches_each=reps + 2,
                          philox_pairs_per_path_step=sum((r >> 1) + 1 for r in ACTIVE[case]), primal_pairs_per_path_step=16)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--driver", nargs=2, metavar=("BOOK", "ROUTE"))
    ap.add_argument("--kernel", choices=sorted(ACTIVE))
    ap.add_argument("--paths", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.driver:
        driver(a.driver[0], a.driver[1], a.paths, a.reps)
    elif a.kernel:
        kernel(a.kernel, a.reps, a.paths)
    else:
        ap.error("--driver BOOK ROUTE or --kernel CASE")
