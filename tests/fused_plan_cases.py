"""The books whose fused-pass plan is pinned in tests/golden/fused_describe.json: what mcx_fused_create decides (straight-line or
interpreted per date, the FastDate flag bits, prefetch pieces, slot size, the cva-date table) and the kernel route of the four
(inject, simulate) pairs, as mcx_fused_describe reports them.  The books are those of test_fused_interpreter.py and the config-3
shape of test_cva_date_kernel.py, at 1,024 main paths: the plan does not depend on the main path count, and the books that need a
pre-simulation keep their 4,096 paths, the size at which the exercise values of berm_book collapse into value polynomials
(FD_EX_VPOLY).  Used by tests/golden/gen_fused_describe_golden.py (writes the file) and test_fused_plan_golden.py (compares)."""
import contextlib

import cases
from mcx import _abi
from test_cva_date_kernel import _irs_book
from test_fused_interpreter import berm_book, bs_book, irs_book

N_MAIN = 1024
PAIRS = [(False, True), (True, True), (False, False), (True, False)]          # (inject, simulate)
AMERICAN = [(5, 100.0)]


def _bench_book():
    """12.5-year quarterly payer swap, 5 sub-steps: the shape bench.py times"""
    ns, model, rm = _irs_book(12.5, True, 0.25, 1.0)
    return ns, model, rm, 4096, 5, cases.E


# id -> (book, options); options: zero_cir = CIR++ starts at zero (the book leaves kf_lean), collapse_pad = SimulationController.collapse_pad
CASES = {
    "bs-npf1": (lambda: bs_book(n_bin=1), {}),
    "bs-npf2": (lambda: bs_book(n_bin=6), {}),
    "bs-npf2-euler": (lambda: bs_book(n_bin=6, euler=True), {}),
    "bs-npf0": (lambda: bs_book(n_bin=12), {}),
    "bs-american-npf1": (lambda: bs_book(n_bin=1, americans=AMERICAN), {}),
    "bs-american-npf2": (lambda: bs_book(n_bin=6, americans=AMERICAN), {}),
    "bs-american-npf0-euler": (lambda: bs_book(n_bin=12, americans=AMERICAN, euler=True), {}),
    "bs-two-americans": (lambda: bs_book(n_bin=0, americans=[(5, 100.0), (4, 106.0)]), {}),
    "bs-two-americans-swapped": (lambda: bs_book(n_bin=0, americans=[(4, 106.0), (5, 100.0)]), {}),
    "bs-2ns": (lambda: bs_book(n_bin=2, n_ns=2), {}),
    "bs-2ns-american": (lambda: bs_book(n_bin=2, n_ns=2, americans=AMERICAN), {}),
    "irs": (lambda: irs_book(bond_opts=1), {}),
    "irs-epe": (lambda: irs_book(bond_opts=1, epe=True), {}),
    "irs-threshold": (lambda: irs_book(bond_opts=1, threshold=0.002), {}),
    "irs-threshold-epe-horizon": (lambda: irs_book(bond_opts=1, epe=True, threshold=0.002, horizon=2.5), {}),
    "irs-horizon": (lambda: irs_book(bond_opts=1, horizon=2.5), {}),
    "irs-2ns": (lambda: irs_book(bond_opts=1, n_ns=2), {}),
    "irs-4ns": (lambda: irs_book(bond_opts=1, n_ns=4), {}),
    "berm": (berm_book, {}),
    "berm-zero-cir": (lambda: berm_book(vol=0.03), {"zero_cir": True, "collapse_pad": -0.25}),
    "bench": (_bench_book, {}),
}
# cases whose plan must carry value polynomials: a shape that loses them pins nothing of that branch
NEED_VPOLY = ("berm", "berm-zero-cir")


@contextlib.contextmanager
def _cir_start_at_zero():
    from mcx.models.cirpp import CIRPPModel
    saved = CIRPPModel._initial_state
    CIRPPModel._initial_state = lambda self: [0.0, 0.0]
    try:
        yield
    finally:
        CIRPPModel._initial_state = saved


def describe(name, hip):
    """{"num_records": n, "inject=i,simulate=s": fused_describe dictionary (arrays as lists)} of a case, JSON-ready"""
    book, opt = CASES[name]
    with _cir_start_at_zero() if opt.get("zero_cir") else contextlib.nullcontext():
        ns, model, rm, n_pre, steps, scheme = book()
        sc = cases.SimulationController(ns, model, rm, N_MAIN, n_pre, steps, scheme, backend=hip)
        if "collapse_pad" in opt:
            sc.collapse_pad = opt["collapse_pad"]
        sc.prepare()                     # descriptors, pre-simulation and regression, mcx_fused_create: no main pass
    assert sc._fused is not None, (name, getattr(hip, "not_fusable_reason", "not fusable"))
    out = {"num_records": int(hip.lib.mcx_fused_num_records(sc._fused.ptr))}
    for inject, simulate in PAIRS:
        d = hip.fused_describe(sc._fused, inject, simulate)
        out[f"inject={int(inject)},simulate={int(simulate)}"] = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in d.items()}
    return out


def has_vpoly(rec):
    return any(f & _abi.FD_EX_VPOLY for f in rec["inject=0,simulate=1"]["flags"])
