"""ctypes mirror of include/mcx.h (the C-ABI boundary).  Pure data-format definitions: no compute here."""
from __future__ import annotations

import ctypes as C

import numpy as np

ABI_VERSION = 6
SELECT_LOST = 1 << 44        # MCX_SELECT_LOST (mcx_select_bracket)
MAX_SLOTS = 8
MAX_Z = 8
MAX_STATE = 16
WIDE_MAX_SLOTS = 32         # MCX_WIDE_MAX_SLOTS: one-factor sub-models of a wide model (mcx_sim_create_wide)
WIDE_MAX_STATE = 64
WIDE_KINDS = (1, 3, 4, 5, 6)  # MCX_MODEL_BS, VASICEK, CIRPP, CIRPP_DET, HW: the kinds a wide model may hold
SLOT_NPARAM = 8
AUX = 8
MAX_BASIS = 6
MAX_STATES = 8
STORAGE_MAX_STATES = 32     # MCX_STORAGE_MAX_STATES: grid states of a gas storage (its own limit; MAX_STATES is the exercise machines')
STORAGE_MAX_KNOTS = 8

SCHEME_EULER, SCHEME_MILSTEIN, SCHEME_ANALYTICAL, SCHEME_QE = 0, 1, 2, 3
MODEL_BS, MODEL_HESTON, MODEL_VASICEK, MODEL_CIRPP, MODEL_CIRPP_DET, MODEL_HW, MODEL_S2F = 1, 2, 3, 4, 5, 6, 7
FLAG_SMOOTHING = 1
# MCX_SIG_*: the model signatures of the path kernels, as mcx_sim_describe reports them
SIG_NAMES = ("GENERIC", "VAS_CIR_E", "BS_A", "BS_E", "HESTON_QE", "HESTON_E", "VAS_E", "VAS_A", "BS_VAS_CIRDET_E", "WIDE")
LSM_MFMA, LSM_F32_CACHE = 1, 2
EV_CASHFLOW, EV_OPTION, EV_EXERCISE, EV_EXPO_POLY, EV_EXPO_BS = 1, 2, 3, 4, 5


class Slot(C.Structure):
    _fields_ = [("kind", C.c_int32), ("state_off", C.c_int32), ("z_off", C.c_int32), ("flags", C.c_int32),
                ("p", C.c_double * SLOT_NPARAM)]


STEP_DTYPE = np.dtype([("dt", "<f8"), ("sqrt_dt", "<f8"), ("t1", "<f8"), ("store_idx", "<i4"), ("chol_idx", "<i4")])
ATOM_DTYPE = np.dtype([("t_idx", "<i4"), ("col", "<i4"), ("a", "<f8"), ("d", "<f8"), ("b", "<f8"), ("c0", "<f8"), ("c1", "<f8")])
TERM_DTYPE = np.dtype([("w", "<f8"), ("atom", "<i4"), ("den", "<i4")])
EVENT_DTYPE = np.dtype([("kind", "<i4"), ("t_idx", "<i4"), ("num_atom", "<i4"), ("x_atom", "<i4"),
                        ("term_begin", "<i4"), ("term_end", "<i4"), ("coeff_off", "<i4"), ("expo_row", "<i4"),
                        ("strike", "<f8"), ("sign", "<f8"), ("aux", "<f8", (4,))])
PRODUCT_DTYPE = np.dtype([("ev_begin", "<i4"), ("ev_end", "<i4"), ("cf_begin", "<i4"), ("cf_end", "<i4"),
                          ("netting_set", "<i4"), ("init_state", "<i4"), ("n_states", "<i4"), ("flags", "<i4")])
ACC_DTYPE = np.dtype([("n", "<f8"), ("shift", "<f8"), ("s1", "<f8"), ("s2", "<f8")])

assert STEP_DTYPE.itemsize == 32 and ATOM_DTYPE.itemsize == 48 and TERM_DTYPE.itemsize == 16
assert EVENT_DTYPE.itemsize == 80 and PRODUCT_DTYPE.itemsize == 32 and ACC_DTYPE.itemsize == 32


class SimDesc(C.Structure):
    _fields_ = [("scheme", C.c_int32), ("n_slots", C.c_int32), ("n_state", C.c_int32), ("n_z", C.c_int32),
                ("n_uniform", C.c_int32), ("n_steps", C.c_int32), ("n_dates", C.c_int32), ("n_chol", C.c_int32),
                ("n_initial_store", C.c_int32), ("flags", C.c_int32),
                ("slots", Slot * MAX_SLOTS),
                ("steps", C.c_void_p), ("chol", C.c_void_p), ("aux", C.c_void_p), ("init_state", C.c_void_p)]


class WideSimDesc(C.Structure):
    """mcx_wide_sim_desc: SimDesc with the slot records behind a pointer ([n_slots] Slot)"""
    _fields_ = [("scheme", C.c_int32), ("n_slots", C.c_int32), ("n_state", C.c_int32), ("n_z", C.c_int32),
                ("n_uniform", C.c_int32), ("n_steps", C.c_int32), ("n_dates", C.c_int32), ("n_chol", C.c_int32),
                ("n_initial_store", C.c_int32), ("flags", C.c_int32),
                ("slots", C.c_void_p),
                ("steps", C.c_void_p), ("chol", C.c_void_p), ("aux", C.c_void_p), ("init_state", C.c_void_p)]


class BookDesc(C.Structure):
    _fields_ = [("n_atoms", C.c_int32), ("n_terms", C.c_int32), ("n_events", C.c_int32), ("n_products", C.c_int32),
                ("n_netting_sets", C.c_int32), ("n_expo_rows", C.c_int32), ("n_basis", C.c_int32), ("n_coeffs", C.c_int32),
                ("want_cfs", C.c_int32), ("want_expo", C.c_int32), ("n_state", C.c_int32), ("n_dates", C.c_int32),
                ("atoms", C.c_void_p), ("terms", C.c_void_p), ("events", C.c_void_p), ("products", C.c_void_p),
                ("coeffs", C.c_void_p)]


class UnsecuredDesc(C.Structure):
    _fields_ = [("n_dates", C.c_int32), ("collateralized", C.c_int32), ("threshold", C.c_double),
                ("row", C.c_void_p), ("delayed", C.c_void_p), ("n_rows", C.c_int32), ("reserved", C.c_int32)]


class FusedNsDesc(C.Structure):
    _fields_ = [("netting_set", C.c_int32), ("n_dates", C.c_int32), ("want_profiles", C.c_int32), ("want_cva", C.c_int32),
                ("threshold", C.c_double), ("recovery", C.c_double),
                ("row", C.c_void_p), ("surv_atoms", C.c_void_p), ("cond_atoms", C.c_void_p)]


class FusedDesc(C.Structure):
    _fields_ = [("n_netting_sets", C.c_int32), ("want_pv", C.c_int32), ("n_expo_rows", C.c_int32), ("reserved", C.c_int32),
                ("row_t_idx", C.c_void_p), ("ns", C.c_void_p)]


E_NOT_FUSABLE = -10
FUSED_MAX_NS = 4
FUSED_MAX_STATEFUL = 4
# mcx_fused_describe (include/mcx.h): MCX_ROUTE_* and the header length MCX_FDESC_HEADER
ROUTE_NONE, ROUTE_LEAN, ROUTE_FUSED = 0, 1, 2
FDESC_HEADER = 16
# MCX_FD_*: flag bits of a date's straight-line record, as mcx_fused_describe reports them
(FD_CASH, FD_EXPO, FD_CVA, FD_PROFILE, FD_CONST_NUM, FD_METRIC, FD_MERGED, FD_EXERCISE, FD_STATE_EXPO, FD_OPTION,
 FD_EX_VPOLY) = (1 << k for k in range(11))
# mcx_eval_book_describe (include/mcx.h): MCX_K2_* kernels, MCX_K2F_* event families, MCX_K2DESC_COUNT entries
K2_SCALAR, K2_CHUNKED, K2_MULTI = 0, 1, 2
K2F_DEN, K2F_EXOTIC, K2F_EXERCISE, K2F_BS_EXPO = 1, 2, 4, 8
K2DESC_COUNT = 6


def ptr(a: np.ndarray | None) -> C.c_void_p:
    """host pointer of a C-contiguous numpy array (None -> NULL)"""
    if a is None:
        return C.c_void_p(0)
    assert a.flags["C_CONTIGUOUS"]
    return C.c_void_p(a.ctypes.data)


# mcx_lsm_job (include/mcx.h)
LSM_DATE_DTYPE = np.dtype([("roll_begin", np.int32), ("roll_end", np.int32), ("num_atom", np.int32), ("x_atom", np.int32),
                           ("degenerate", np.int32), ("reserved", np.int32), ("coeff_off", np.int64, (2,)),
                           ("shift", np.float64), ("scale", np.float64), ("x0", np.float64)])
assert LSM_DATE_DTYPE.itemsize == 64
LSM_JOB_DTYPE = np.dtype([("product", np.int32), ("roll_begin", np.int32), ("roll_end", np.int32), ("num_atom", np.int32),
                          ("x_atom", np.int32), ("reserved", np.int32), ("w_offset", np.int64), ("shift", np.float64),
                          ("scale", np.float64)], align=True)

LSM_SOLVE_JOB_DTYPE = np.dtype([("shift", np.float64), ("scale", np.float64), ("x0", np.float64), ("coeff_off", np.int64, (2,)),
                                ("degenerate", np.int32), ("reserved", np.int32)], align=True)
assert LSM_SOLVE_JOB_DTYPE.itemsize == 48

TANGENT_NP = 4          # MCX_TANGENT_NP: model parameters per forward-mode pass (csrc/kt_book.hip)
# mcx_tangent_lsm_job: one (stateless product, regression date) pair of mcx_tangent_lsm_batch
TANGENT_LSM_JOB_DTYPE = np.dtype([("product", "<i4"), ("first_event", "<i4"), ("num_atom", "<i4"), ("x_atom", "<i4"),
                                  ("shift", "<f8"), ("scale", "<f8")])
assert TANGENT_LSM_JOB_DTYPE.itemsize == 32
# mcx_tangent_paths_wide(h, sim, h_dslot, h_dinit, h_daux, h_dchol, seed, path_offset, n_paths, d_paths, d_dpaths, ld, d_inject_z,
# n_active_out, stream); mcx_tangent_paths_wide_hw takes the same list
TANGENT_PATHS_WIDE_ARGTYPES = [C.c_void_p] * 6 + [C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                                  C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]

# gas storage (include/mcx.h "K6"): mcx_storage_date, mcx_storage_desc, mcx_storage_lsm_date, mcx_storage_op
STORAGE_DATE_DTYPE = np.dtype([("vmin", "<f8"), ("step", "<f8"), ("next_vmin", "<f8"), ("next_vmax", "<f8"), ("next_scale", "<f8"),
                               ("period", "<f8"), ("c_inj", "<f8"), ("c_wd", "<f8"),
                               ("inj_x", "<f8", (STORAGE_MAX_KNOTS,)), ("inj_r", "<f8", (STORAGE_MAX_KNOTS,)),
                               ("wd_x", "<f8", (STORAGE_MAX_KNOTS,)), ("wd_r", "<f8", (STORAGE_MAX_KNOTS,)),
                               ("coeff_off", "<i8"), ("n_inj", "<i4"), ("n_wd", "<i4"), ("num_atom", "<i4"), ("x_atom", "<i4"),
                               ("is_last", "<i4"), ("reserved", "<i4")])
assert STORAGE_DATE_DTYPE.itemsize == 8 * 8 + 4 * 8 * STORAGE_MAX_KNOTS + 8 + 6 * 4


class StorageDesc(C.Structure):
    _fields_ = [("n_states", C.c_int32), ("n_dates", C.c_int32), ("netting_set", C.c_int32), ("reserved", C.c_int32),
                ("dates", C.c_void_p), ("trans", C.c_void_p)]


STORAGE_LSM_DATE_DTYPE = np.dtype([("roll_date", "<i4"), ("num_atom", "<i4"), ("x_atom", "<i4"), ("degenerate", "<i4"),
                                   ("coeff_off", "<i8", (2,)), ("shift", "<f8"), ("scale", "<f8"), ("x0", "<f8")])
STORAGE_OP_DTYPE = np.dtype([("kind", "<i4"), ("index", "<i4"), ("num_atom", "<i4"), ("x_atom", "<i4"), ("coeff_off", "<i8")])
assert STORAGE_LSM_DATE_DTYPE.itemsize == 56 and STORAGE_OP_DTYPE.itemsize == 24
STORAGE_OP_ACTION, STORAGE_OP_EXPOSURE = 0, 1
# mcx_storage_lsm_job: one (storage, date) pair of the product-batched backward induction (mcx_storage_lsm_step_batch,
# mcx_storage_lsm_solve_batch, mcx_storage_lsm_run_batch)
STORAGE_LSM_JOB_DTYPE = np.dtype([("storage", "<i4"), ("roll_date", "<i4"), ("num_atom", "<i4"), ("x_atom", "<i4"), ("degenerate", "<i4"),
                                  ("reserved", "<i4"), ("coeff_off", "<i8", (2,)), ("w_old", "<i8"), ("w_new", "<i8"),
                                  ("shift", "<f8"), ("scale", "<f8"), ("x0", "<f8")])
assert STORAGE_LSM_JOB_DTYPE.itemsize == 80
