#!/usr/bin/env python3
"""tests/golden/large_cva_aad.npz: the reference's large-netting-set CVA book at 72 products (tests/large_cva_cases.py SMALL) with
differentiate=True — its recorded draws, its CVA and its autograd gradients.  Run where the reference is importable (as
gen_golden.py, whose draw recorder and class imports are reused):   python tests/golden/gen_large_cva_aad_golden.py
The fixture holds z_pre, z_main, param_names, result_* and grad_* only: no paths, no per-product dumps.  The credit slot is
deterministic CIR++ (cirpp.py:155-172 there): its step never reads its normal, so that column of the draws is stored as zeros —
incompressible noise nobody consumes would push the file over the size limit of a committed fixture."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import gen_golden as ref                 # puts the reference on sys.path; `ref` is the namespace of its classes
import large_cva_cases


def main():
    torch.set_num_threads(4)
    cfg = large_cva_cases.SMALL
    ns, model, rm = large_cva_cases.build(cfg["num_europeans"], cfg["num_bonds"], cfg["num_swaps"], cfg["exposure_timeline"], lib=ref)
    sc = ref.SimulationController(netting_sets=ns, model=model, risk_metrics=rm, num_paths_mainsim=cfg["n_main"],
                                  num_paths_presim=cfg["n_pre"], num_steps=cfg["num_steps"],
                                  simulation_scheme=ref.SimulationScheme.EULER, differentiate=True)
    with ref.DrawRecorder() as rec:
        res = sc.run_simulation()
    half = len(rec.normals) // 2          # pre-simulation first, both engines draw equally often (gen_golden.run_controller_case)
    out = {"z_pre": np.stack(rec.normals[:half], axis=0), "z_main": np.stack(rec.normals[half:], axis=0),
           "param_names": np.array(res.model_param_names)}
    assert out["z_pre"].shape[1:] == (cfg["n_pre"], 3) and out["z_main"].shape[1:] == (cfg["n_main"], 3)
    out["z_pre"][:, :, 2] = 0.0           # slot 2 = deterministic credit: drawn, never read
    out["z_main"][:, :, 2] = 0.0
    for ns_i, per_ns in enumerate(res.results):
        for m_i, m in enumerate(per_ns):
            out[f"result_{ns_i}_{m_i}"] = np.array([[float(v[0]), float(v[1])] for v in m])
    for ns_i, per_ns in enumerate(res.derivatives):
        for m_i, m in enumerate(per_ns):
            out[f"grad_{ns_i}_{m_i}"] = np.array([[np.nan if d is None else float(d) for d in ev] for ev in m])
    path = os.path.join(HERE, "large_cva_aad.npz")
    np.savez_compressed(path, **out)
    print(f"large_cva_aad: {len(sc.products)} products, wrote {os.path.getsize(path) / 1024:.0f} KiB;",
          {k: v.tolist() for k, v in out.items() if k.startswith(("result_", "grad_"))})


if __name__ == "__main__":
    main()
