#!/usr/bin/env python3
"""Timings of the storage's sensitivities on one GPU (profiles/storage_aad_*; run under `rocprofv3 --kernel-trace --stats --` for
the per-kernel device times):

  step N    differentiate=True on the 10-state storage with a cubic regression of tools/prof_storage.py (S = 10, K = 4, 64 daily
            action dates) with N pre-simulation and N main paths: per backward date one kts_step launch per pass of four
            parameters, per pass one kts_eval launch (next to k6_step / k6_eval of the base run inside the same call)
  storage2  run_simulation() of the reference's `storage2` scenario (454 action dates, cubic regression, 2,000 + 4,000 paths)
            with and without differentiate=True, three runs each, next to the reference's CPU seconds for the differentiated run
            (tests/golden/storage_anchors_aad.npz) and its PV gradient

    python tools/prof_storage_aad.py step 4000 | step 262144 | storage2"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "montecarlo-risk-engine_amd"), os.path.join(ROOT, "tests")]

import storage_cases                                                                    # noqa: E402
from mcx import _native                                                                 # noqa: E402
from mcx.common.enums import SimulationScheme                                           # noqa: E402
from mcx.controller.controller import SimulationController                             # noqa: E402
from mcx.maths.regression import PolyomialRegression                                    # noqa: E402


def step_timing(be, mod, n):
    p = storage_cases._daily_store(mod, 10, 64.0, [(0.0, 20.0, 0.0, 12.0), (20.0, 40.0, 2.0, 10.0), (40.0, 65.0, 0.0, 6.0)])
    model = mod["SchwartzTwoFactorModel"](0.0, [0.0, 16.0, 40.0, 64.0], [30.0, 32.0, 29.0, 31.0], rate=0.002, short_term_mean_reversion=0.3,
                                          short_term_vol=0.12, long_term_drift=0.001, long_term_vol=0.04, rho=0.3, asset_id="gas")
    rm = mod["RiskMetrics"]([mod["PVMetric"](), mod["EPEMetric"]()], exposure_timeline=np.arange(0.0, 65.0, 8.0))
    out = dict(what="differentiate=True, S=10, K=4, 64 action dates", n_pre=n, n_main=n, runs=[])
    for _ in range(3):
        sc = SimulationController([mod["NettingSet"](name="st", products=[p])], model, rm, n, n, 1, SimulationScheme.ANALYTICAL, True,
                                  regression_function=PolyomialRegression(degree=3), backend=be)
        t0 = time.perf_counter()
        sc.run_simulation()
        be.synchronize()
        out["runs"].append(dict(seconds=time.perf_counter() - t0, timings=sc.timings))
        sc.release_device_buffers()
    return out


def storage2_timing(be, mod):
    g, ga = storage_cases.load_golden("storage_anchors"), storage_cases.load_golden("storage_anchors_aad")
    out = dict(what="storage2 run_simulation()", n_main=2000, n_pre=4000, reference_seconds_cpu_differentiated=float(ga["storage2_aad_seconds"]),
               reference_seconds_cpu_plain=float(g["storage2_seconds"]), reference_cpu=str(ga["cpu"]),
               reference_pv_grad=ga["storage2_pv_grad"].tolist(), runs=[])
    for differentiate in (False, True, False, True, False, True):
        p, model = storage_cases.anchor_scenario(g, "storage2", mod)
        sc = SimulationController([mod["NettingSet"](name="st", products=[p])], model, mod["RiskMetrics"](metrics=[mod["PVMetric"]()]), 2000, 4000, 1,
                                  SimulationScheme.ANALYTICAL, differentiate, regression_function=PolyomialRegression(degree=3), backend=be)
        t0 = time.perf_counter()
        res = sc.run_simulation()
        be.synchronize()
        run = dict(differentiate=differentiate, seconds=time.perf_counter() - t0, pv=res.results[0][0][0][0], timings=sc.timings)
        if differentiate:
            run["pv_grad"] = [float(v) for v in res.derivatives[0][0][0]]
        out["runs"].append(run)
        sc.release_device_buffers()
    return out


def main():
    what = sys.argv[1:] or ["storage2"]
    be, mod = _native.HipBackend(0), storage_cases.mcx_classes()
    if what[0] == "step":
        print(json.dumps(step_timing(be, mod, int(what[1])), default=float), flush=True)
    else:
        print(json.dumps(storage2_timing(be, mod), default=float), flush=True)


if __name__ == "__main__":
    main()
