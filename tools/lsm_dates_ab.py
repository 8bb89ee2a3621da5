#!/usr/bin/env python3
"""Date-batched LSM against today's routes on the bench workload's own book (one payer swap, exposure regression at 51 dates).

One process = one route: warm with a small and one full-size pre-simulation, then time `--reps` pre-simulations.  Per repetition
the line holds the wall time of the pre-simulation (paths + regression, ends in a device synchronise) and of the regression alone
(the route functions of the controller between two synchronises).  Interleave processes of the two routes to see the spread:

    for r in 1 2 3; do python tools/lsm_dates_ab.py --route off; python tools/lsm_dates_ab.py --route on; done

Under `rocprofv3 --kernel-trace --stats -- python tools/lsm_dates_ab.py --route on --reps 5` the per-kernel averages are the
device times (k3_dates + k3_finish_solve_batch against 51 x (k3_step_valu + k3_finish_solve))."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
from mcx import _native


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("on", "off"), required=True)
    ap.add_argument("--presim", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    be = _native.HipBackend(0)

    def presim(n_pre):
        sc = bench.build_controller(4096, n_pre, be)
        sc.date_batched_lsm = args.route == "on"
        spent = [0.0]
        for fn in ("_perform_regression_routes", "_perform_regression_dates"):
            inner = getattr(sc, fn)

            def timed(*a, _inner=inner, **k):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                out = _inner(*a, **k)
                torch.cuda.synchronize(); spent[0] += time.perf_counter() - t0
                return out
            setattr(sc, fn, timed)
        torch.cuda.synchronize()
        sc.prepare()
        torch.cuda.synchronize()
        return sc, spent[0]

    presim(4096)
    presim(args.presim)
    for rep in range(args.reps):
        sc, reg = presim(args.presim)
        print(json.dumps(dict(route=args.route, presim_paths=args.presim, rep=rep, lsm_routes=sc.lsm_routes,
                              presim_and_regression_ms=1e3 * sc.prepare_timings["presim_and_regression"], regression_ms=1e3 * reg)), flush=True)


if __name__ == "__main__":
    main()
