#!/usr/bin/env python3
"""In-process A/B of the two storage pre-simulation routes on the PV book of tools/large_book.py: a fresh controller per repetition
(as large_book.py builds one), `batch_storage_lsm` alternating off / on, so that both routes see the same process, allocator and
clock state.  Per repetition one JSON line: run_s, timings["preprocessing"], the wall time of _perform_regression (synchronised),
the summed and the longest schedule length of the storages.

    python tools/large_book_storage_ab.py pv 100 [scale]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.join(ROOT, "montecarlo-risk-engine_amd")]
import numpy as np
import large_book as LB
from mcx import _native
from mcx.controller.controller import SimulationController as SC

acc = {}
def wrap(name):
    orig = getattr(SC, name)
    def f(self, *a, **k):
        t0 = time.perf_counter()
        try:
            return orig(self, *a, **k)
        finally:
            self.backend.synchronize()
            acc[name] = acc.get(name, 0.0) + time.perf_counter() - t0
    setattr(SC, name, f)
wrap("_perform_regression")

be = _native.HipBackend(0)
ids = [f"asset_{k}" for k in range(4)]
book, n_st, scale = sys.argv[1], int(sys.argv[2]), float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
mult = 10 if book == "pv" else 1
counts = [max(1, int(round(c * mult * scale))) for c in (3940, 100, 100, 200, 400, 180, 70)]
for rep in range(9):
    batch = rep % 2 == 1
    corr = np.full((4, 4), 0.35); np.fill_diagonal(corr, 1.0)
    market = LB.BlackScholesMulti(0.0, 0.03, ids, [95.0 + 7.5 * k for k in range(4)], [0.18 + 0.03 * k for k in range(4)], corr)
    products = LB.build_mixed_book(ids, *counts) + LB.build_storages(ids, n_st)
    ns = LB.NettingSet(name="b", products=products)
    sc = SC([ns], market, LB.RiskMetrics([LB.PVMetric()]), 1000, 1000, 1, LB.SimulationScheme.ANALYTICAL, backend=be)
    sc.batch_storage_lsm = batch
    acc.clear()
    t0 = time.perf_counter(); res = sc.run_simulation(); be.synchronize(); t1 = time.perf_counter()
    L = [len(sc._regression_schedule(i, sc.products[i])) for i in sorted(sc._storage_meta)]
    print(json.dumps(dict(book=book, storages=n_st, rep=rep, route=sc.storage_lsm_route, run_s=t1 - t0, preprocessing=sc.timings["preprocessing"],
                          perform_regression_s=acc.get("_perform_regression"),
                          sum_L=sum(L), max_L=max(L), pv=float(res.results[0][0][0][0]))), flush=True)
