#!/usr/bin/env python3
"""Gas-storage timings on one GPU (profiles/storage_*.json; run under `rocprofv3 --kernel-trace --stats --` for the per-kernel split):

  step      the backward induction of a 10-state storage with a cubic regression (S = 10, K = 4; the `storage_shift` case of
            tests/storage_cases.py stretched to 64 daily action dates) at 4,000 and 262,144 pre-simulation paths: wall time of
            mcx_storage_lsm_run per regression date (step + finish/solve launches, one synchronisation at the end)
  storage2  run_simulation() of the reference's `storage2` scenario (454 action dates, tests/golden/storage_anchors.npz) at
            2,000 + 4,000 and at 262,144 + 262,144 paths, first (cold) and second run

  batch:N_PRE:N   the product-batched induction (mcx_storage_lsm_run_batch) of N copies of the `step` storage in one netting set at
            N_PRE paths: wall time per step of the batch (a step = one k6_step_batch + one k6_finish_solve_batch launch for all N
            storages) next to the per-storage route's N mcx_storage_lsm_run calls on the same book

    python tools/prof_storage.py [step] [storage2] [batch:1000:100] [batch:262144:10]"""
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


def step_timing(be, mod, n_pre):
    p = storage_cases._daily_store(mod, 10, 64.0, [(0.0, 20.0, 0.0, 12.0), (20.0, 40.0, 2.0, 10.0), (40.0, 65.0, 0.0, 6.0)])
    model = mod["SchwartzTwoFactorModel"](0.0, [0.0, 16.0, 40.0, 64.0], [30.0, 32.0, 29.0, 31.0], rate=0.002, short_term_mean_reversion=0.3,
                                          short_term_vol=0.12, long_term_drift=0.001, long_term_vol=0.04, rho=0.3, asset_id="gas")
    sc = SimulationController([mod["NettingSet"](name="st", products=[p])], model, mod["RiskMetrics"]([mod["PVMetric"]()]), 1024, n_pre, 1,
                              SimulationScheme.ANALYTICAL, False, regression_function=PolyomialRegression(degree=3), backend=be)
    walls = []
    orig = be.storage_lsm_run

    def timed(*a, **k):
        be.synchronize()
        t0 = time.perf_counter()
        out = orig(*a, **k)
        walls.append((time.perf_counter() - t0, len(a[2])))
        return out

    be.storage_lsm_run = timed
    try:
        for _ in range(4):
            sc.run_simulation()
    finally:
        del be.storage_lsm_run
    best, n_dates = min(walls[1:])
    return dict(what="mcx_storage_lsm_run", S=10, K=4, n_pre=n_pre, regression_dates=n_dates, wall_ms=best * 1e3, us_per_date=best / n_dates * 1e6)


def batch_timing(be, mod, n_pre, n_storages):
    stores = []
    for j in range(n_storages):
        p = storage_cases._daily_store(mod, 10, 64.0, [(0.0, 20.0, 0.0, 12.0), (20.0, 40.0, 2.0, 10.0), (40.0, 65.0, 0.0, 6.0)])
        p.name = f"store{j}"
        stores.append(p)
    model = mod["SchwartzTwoFactorModel"](0.0, [0.0, 16.0, 40.0, 64.0], [30.0, 32.0, 29.0, 31.0], rate=0.002, short_term_mean_reversion=0.3,
                                          short_term_vol=0.12, long_term_drift=0.001, long_term_vol=0.04, rho=0.3, asset_id="gas")
    sc = SimulationController([mod["NettingSet"](name="st", products=stores)], model, mod["RiskMetrics"]([mod["PVMetric"]()]), 1024, n_pre, 1,
                              SimulationScheme.ANALYTICAL, False, regression_function=PolyomialRegression(degree=3), backend=be)
    walls = {"storage_lsm_run_batch": [], "storage_lsm_run": []}

    def timed(name):
        orig = getattr(be, name)

        def call(*a, **k):
            be.synchronize()
            t0 = time.perf_counter()
            out = orig(*a, **k)
            walls[name].append(time.perf_counter() - t0)
            return out
        return call

    for name in walls:
        setattr(be, name, timed(name))
    pvs = {}
    try:
        for batch in (True, False):
            sc.batch_storage_lsm = batch
            for _ in range(3):
                pvs[batch] = sc.run_simulation().results[0][0][0]
    finally:
        for name in walls:
            delattr(be, name)
    n_steps = len(sc._regression_schedule(0, sc.products[0]))
    best_batch = min(walls["storage_lsm_run_batch"][1:])
    per = np.array(walls["storage_lsm_run"]).reshape(3, n_storages).sum(axis=1)
    best_single = float(per[1:].min())
    return dict(what="mcx_storage_lsm_run_batch", S=10, K=4, n_pre=n_pre, storages=n_storages, steps=n_steps, batch_wall_ms=best_batch * 1e3,
                batch_us_per_step=best_batch / n_steps * 1e6, per_storage_route_wall_ms=best_single * 1e3,
                per_storage_route_us_per_date=best_single / (n_steps * n_storages) * 1e6, same_pv=bool(pvs[True] == pvs[False]))


def storage2_timing(be, mod, n_main, n_pre):
    g = storage_cases.load_golden("storage_anchors")
    out = dict(what="storage2 run_simulation()", n_main=n_main, n_pre=n_pre, reference_seconds_cpu=float(g["storage2_seconds"]),
               reference_cpu=str(g["cpu"]), runs=[])
    for rep in range(3):
        p, model = storage_cases.anchor_scenario(g, "storage2", mod)
        sc = SimulationController([mod["NettingSet"](name="st", products=[p])], model, mod["RiskMetrics"]([mod["PVMetric"]()]), n_main, n_pre, 1,
                                  SimulationScheme.ANALYTICAL, False, regression_function=PolyomialRegression(degree=3), backend=be)
        t0 = time.perf_counter()
        res = sc.run_simulation()
        be.synchronize()
        pv, se = res.results[0][0][0]
        out["runs"].append(dict(seconds=time.perf_counter() - t0, pv=pv, mc_error=se, timings=sc.timings, prepare=sc.prepare_timings))
        sc.release_device_buffers()
    return out


def main():
    what = sys.argv[1:] or ["step", "storage2"]
    be, mod = _native.HipBackend(0), storage_cases.mcx_classes()
    if "step" in what:
        for n_pre in (4000, 262144):
            print(json.dumps(step_timing(be, mod, n_pre), default=float), flush=True)
    for w in what:
        if w.startswith("batch:"):
            _, n_pre, n_storages = w.split(":")
            print(json.dumps(batch_timing(be, mod, int(n_pre), int(n_storages)), default=float), flush=True)
    if "storage2" in what:
        for n_main, n_pre in ((2000, 4000), (262144, 262144)):
            print(json.dumps(storage2_timing(be, mod, n_main, n_pre), default=float), flush=True)


if __name__ == "__main__":
    main()
