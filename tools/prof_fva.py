#!/usr/bin/env python3
"""Device time of the FVA kernel (csrc/k4_fva.hip, mcx_reduce_fva) next to mcx_reduce_xva and mcx_reduce_cva on the same inputs,
and the wall time of a run with FVAMetric on the native route against the metric's host form.

    python tools/prof_fva.py kernel [--paths N] [--dates E] [--reps R]
    python tools/prof_fva.py e2e --route native|host [--paths N] [--dates E]

kernel (default): the payer-swap book of tests/xva_cases.py (Vasicek + CIR++ counterparty + CIR++ own name) at N paths and E
exposure dates is simulated once; mcx_reduce_fva (three records, one launch + k_finish_acc), mcx_reduce_xva (five records, one
launch + k_finish_acc) and mcx_reduce_cva (one record: k4_cva_paths / k4_cva_paths_v<2>, k4_vector, k_finish_acc) then run on the
SAME exposure block and paths with both names set, plain and with a threshold.  Each is warmed (3 calls), then R calls are timed with
device events around the call (host staging of the ids and weights and the copy of the records included: that is what a caller
pays).  One JSON line per (entry point, descriptor): ms per call (median, min, max), the algorithmic bytes — (E - 1) x N x 8 for the
exposure rows read plus as much per state column the atoms read (two for fva and xva, one for cva, which also writes and re-reads
its N x 8 scratch vector) — and the TB/s they give.
e2e: run_simulation() of the same book with FVAMetric through mcx_reduce_fva (native) or through evaluate_numerically (host: a
subclass with _native = False), wall time of three runs after a warm-up run.

One process start per invocation: repeat the command for the spread between starts.  Kernel names for
`rocprofv3 --kernel-trace --stats -- python tools/prof_fva.py kernel`: k4_fva, k4_xva, k4_cva_paths, k4_cva_paths_v<2>, k4_vector."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "montecarlo-risk-engine_amd"), os.path.join(ROOT, "tests")]

import numpy as np
import torch

import xva_cases as xc
from mcx import _native
from mcx.metrics.bcva_metric import BilateralCVAMetric
from mcx.metrics.fva_metric import FVAMetric
from mcx.plan import UnsecuredSpec

BORROW_CURVE = {0.5: 0.012, 1.0: 0.015, 1.75: 0.02, 5.0: 0.025}
LEND_CURVE = {0.3: 0.004, 1.25: 0.006, 2.0: 0.009}


class HostFVA(FVAMetric):
    _native = False


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


def kernel(be, a):
    tl = np.linspace(0.0, 2.5, a.dates)
    fva = FVAMetric(BORROW_CURVE, LEND_CURVE, counterparty_id="cp", own_id="own")
    sc = xc.controller(be, [BilateralCVAMetric("cp", "own", xc.R_CP, xc.R_OWN), fva], n_main=a.paths, n_pre=4096, timeline=tl)
    sc.run_simulation()
    (cp, _), (own, _) = sc._xva_atoms[0]
    cp_surv, own_surv = sc._fva_atoms[1]
    paths, expo = sc.last_state["paths"], sc.last_state["expo"][0]
    rows = sc.metric_exposure_indices.numpy()
    cell = (a.dates - 1) * a.paths * 8
    for tag, h in (("plain", 0.0), ("threshold", xc.THRESHOLD)):
        u = UnsecuredSpec(rows, None, h, False)
        runs = (("mcx_reduce_fva", lambda: be.reduce_fva(sc.book, u, cp_surv, own_surv, fva.w_borrow, fva.w_lend, expo, paths), 3 * cell),
                ("mcx_reduce_xva", lambda: be.reduce_xva(sc.book, u, cp, xc.R_CP, own, xc.R_OWN, expo, paths), 3 * cell),
                ("mcx_reduce_cva", lambda: be.reduce_cva(sc.book, u, cp[0], cp[1], xc.R_CP, expo, paths), 2 * cell + 2 * a.paths * 8))
        for name, fn, nbytes in runs:
            med, lo, hi = timed(fn, a.reps)
            print(json.dumps(dict(entry=name, descriptor=tag, paths=a.paths, dates=a.dates, ms_per_call=round(med, 4), ms_min=round(lo, 4),
                                  ms_max=round(hi, 4), algorithmic_bytes=nbytes, tb_per_s=round(nbytes / (med * 1e-3) / 1e12, 3))), flush=True)


def e2e(be, a):
    cls = FVAMetric if a.route == "native" else HostFVA
    sc = xc.controller(be, [cls(BORROW_CURVE, LEND_CURVE, counterparty_id="cp", own_id="own")], n_main=a.paths, n_pre=4096,
                       timeline=np.linspace(0.0, 2.5, a.dates))
    sc.materialize = False
    res = sc.run_simulation()
    torch.cuda.synchronize()
    walls, metrics = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        res = sc.run_simulation()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        metrics.append(sc.timings.get("metrics"))
    print(json.dumps(dict(route=a.route, paths=a.paths, dates=a.dates, fused=sc._fused is not None, run_simulation_s=[round(w, 4) for w in walls],
                          metrics_s=[round(m, 4) for m in metrics], fva=[float(v) for v, _ in res.results[0][0]])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="kernel", choices=["kernel", "e2e"])
    ap.add_argument("--route", default="native", choices=["native", "host"])
    ap.add_argument("--paths", type=int, default=262144)
    ap.add_argument("--dates", type=int, default=51)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    be = _native.HipBackend(0)
    (kernel if a.mode == "kernel" else e2e)(be, a)


if __name__ == "__main__":
    main()
