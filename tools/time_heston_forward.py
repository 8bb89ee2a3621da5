#!/usr/bin/env python3
"""run_simulation() wall time of a Heston exercise book with differentiate=True: the forward-mode book pass on
mcx_tangent_paths_heston (SimulationController.tangent_heston = True, 2 passes) against bump-and-revalue (False, 14 bumped runs).

    python tools/time_heston_forward.py --driver        # fresh processes, the two routes interleaved, three repetitions
    python tools/time_heston_forward.py --route forward # one process: warm-up at 4,096 paths, one full-size run, then the timed run

The book: an American put on Heston QE, 12 exercise dates, PV, 262,144 + 262,144 paths, Philox draws.  The timed figure is the host
clock around run_simulation() of a fresh controller, the device synchronised before and after.  One JSON line per process."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "montecarlo-risk-engine_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def controller(be, n, forward):
    import cases
    model = cases.HestonModel(0.0, 100.0, 0.03, 0.3, -0.6, 2.0, 0.06, 0.05)
    prod = cases.AmericanOption(cases.Equity(), 3.0, 12, 100.0, cases.OptionType.PUT)
    ns = [cases.NettingSet(name="american", products=[prod])]
    sc = cases.SimulationController(ns, model, cases.RiskMetrics([cases.PVMetric()]), n, n, 2, cases.Q, differentiate=True, backend=be)
    sc.tangent_heston = forward
    return sc


def one_process(route, n):
    from mcx import _native
    be = _native.HipBackend(0)
    forward = route == "forward"
    out = {}
    for label, paths in (("warm_small", 4096), ("warm_full", n), ("timed", n)):
        sc = controller(be, paths, forward)
        be.synchronize()
        t0 = time.perf_counter()
        res = sc.run_simulation()
        be.synchronize()
        out[label + "_ms"] = 1e3 * (time.perf_counter() - t0)
        assert sc.timings["tangent"] is forward, sc.timings
    out.update(route=route, paths=n, passes=sc.timings.get("forward_mode_passes", sc.timings.get("bumped_passes")),
               pv=float(res.results[0][0][0][0]), grad=[float(x) for x in res.derivatives[0][0][0]])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--driver", action="store_true")
    ap.add_argument("--route", choices=["forward", "bump"], default="forward")
    ap.add_argument("--paths", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if not a.driver:
        return one_process(a.route, a.paths)
    for _ in range(a.reps):
        for route in ("forward", "bump"):
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", route, "--paths", str(a.paths)], timeout=300).returncode
            if rc != 0:                       # a process that failed ends the series: nothing more is started on the device
                sys.exit(rc)


if __name__ == "__main__":
    main()
