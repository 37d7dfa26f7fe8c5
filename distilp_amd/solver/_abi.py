"""The C ABI of libhalda (include/halda.h, and include/halda_boxes.h beside it) as ctypes declarations: every
struct, in header order, and the prototype of every function. `_libhalda.load_library` applies PROTOTYPES and
BOXES_PROTOTYPES to the library it opens, so no call can reach a function with ctypes' default `int` arguments
and result. tests/test_abi.py compiles halda.h and compares every struct's size and field offsets, and every
prototype's arity and result type, with this module; tests/test_boxes.py does the same for halda_boxes.h.
"""

from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p


def _ptrs(*names):
    """Pointer members (typed in the header; here addresses: int, None or a ctypes pointer alike)."""
    return [(n, c_void_p) for n in names]


class HaldaBatchC(ctypes.Structure):
    _fields_ = ([(n, c_int32) for n in ("n_inst", "max_cols", "max_R1", "max_tab", "max_tab_kc")]
                + _ptrs("n_cols", "n_rows", "csr_off", "col_off", "row_off", "row_ptr", "col_idx", "val", "c", "col_lb",
                        "col_ub", "row_lb", "row_ub", "integrality")
                + [("mip_rel_gap", c_double), ("mip_abs_gap", c_double), ("time_limit", c_double)] + _ptrs("x0", "y0"))


class HaldaResultC(ctypes.Structure):
    _fields_ = _ptrs("status", "x", "obj_lin", "dual_bound", "gap", "nodes")


class HaldaModelC(ctypes.Structure):
    _fields_ = [("f_q_b1", c_double), ("f_out_b1", c_double), ("has_f_q", c_int32), ("has_f_out", c_int32),
                ("b_prime", c_double), ("b_layer", c_double), ("b_in", c_double), ("b_out", c_double), ("V", c_double),
                ("L", c_int32)]


F64_FIELDS = ("scpu_b1", "sgpu_b1", "T_cpu", "T_gpu", "t_kvcpy_cpu", "t_kvcpy_gpu", "t_ram2vram", "t_vram2ram",
              "t_comm", "s_disk")
# the profiles' integer byte counts, held as float64 (ABI 3): exact below 2^53, so the reference's integer
# sums and differences of them are exact in the kernels' double arithmetic
BYTE_FIELDS = ("d_avail_ram", "c_cpu", "c_gpu", "d_avail_cuda", "d_avail_metal", "swap")


class HaldaFleetsC(ctypes.Structure):
    _fields_ = ([("n_fleets", c_int32), ("min_devices", c_int32), ("max_devices", c_int32)]
                + _ptrs("dev_off", "os_class", "flags", *F64_FIELDS, *BYTE_FIELDS))


class HaldaFleetResultC(ctypes.Structure):
    _fields_ = _ptrs("best_k", "obj_value", "w", "n", "obj_by_k", "status", "x", "c", "x_off")


class HaldaSubfleetsC(ctypes.Structure):
    _fields_ = ([("n_items", c_int32), ("min_devices", c_int32), ("max_devices", c_int32)]
                + _ptrs("parent", "sub_off", "sub_idx"))


class HaldaPlansC(ctypes.Structure):
    _fields_ = _ptrs("k", "w", "n")


class HaldaPlanResultC(ctypes.Structure):
    _fields_ = _ptrs("status", "obj_value", "cycle", "bottleneck", "reason", "x", "c", "x_off")


class HaldaBoundsC(ctypes.Structure):
    _fields_ = _ptrs("w_min", "w_max")


class HaldaBoxC(ctypes.Structure):  # halda_box: halda_bounds and the n columns' two arrays
    _fields_ = _ptrs("w_min", "w_max", "n_min", "n_max")


class HaldaBoxesC(ctypes.Structure):  # include/halda_boxes.h halda_boxes: n_box planes of halda_box's arrays
    _fields_ = [("n_box", c_int32)] + _ptrs("w_min", "w_max", "n_min", "n_max")


class HaldaBudgetC(ctypes.Structure):
    _fields_ = _ptrs("w0", "w_min", "w_max") + [("max_p", c_int32)]


class HaldaFrontierC(ctypes.Structure):
    _fields_ = [("n_devices", c_int64)] + _ptrs("status", "obj", "moved", "w", "n")


class HaldaChangeC(ctypes.Structure):
    _fields_ = _ptrs("w0", "w_min", "w_max") + [("max_p", c_int32), ("max_deficit", c_int32)]


class HaldaChangeFrontierC(ctypes.Structure):
    _fields_ = [("n_devices", c_int64)] + _ptrs("status", "obj", "loaded", "released", "w", "n")


class HaldaSubsetsC(ctypes.Structure):
    _fields_ = [("max_drop", c_int32)] + _ptrs("keep_mask")


class HaldaSubsetFrontierC(ctypes.Structure):
    _fields_ = _ptrs("status", "obj", "dropped_mask", "best_k")


class HaldaChangeSubsetsC(ctypes.Structure):
    _fields_ = (_ptrs("w0", "w_min", "w_max") + [("min_drop", c_int32), ("max_drop", c_int32), ("max_p", c_int32)]
                + _ptrs("keep_mask"))


class HaldaChangeSubsetFrontierC(ctypes.Structure):
    _fields_ = _ptrs("status", "obj", "dropped_mask", "loaded", "released", "w", "n")


# Python class -> the header's typedef, in header order
STRUCTS = {HaldaBatchC: "halda_batch", HaldaResultC: "halda_result", HaldaModelC: "halda_model",
           HaldaFleetsC: "halda_fleets", HaldaFleetResultC: "halda_fleet_result", HaldaSubfleetsC: "halda_subfleets",
           HaldaPlansC: "halda_plans", HaldaPlanResultC: "halda_plan_result", HaldaBoundsC: "halda_bounds",
           HaldaBoxC: "halda_box", HaldaBudgetC: "halda_budget", HaldaFrontierC: "halda_frontier",
           HaldaChangeC: "halda_change", HaldaChangeFrontierC: "halda_change_frontier", HaldaSubsetsC: "halda_subsets",
           HaldaSubsetFrontierC: "halda_subset_frontier", HaldaChangeSubsetsC: "halda_change_subsets",
           HaldaChangeSubsetFrontierC: "halda_change_subset_frontier"}

_vp, _vpp, _dp, _ip = c_void_p, POINTER(c_void_p), POINTER(c_double), POINTER(c_int)
_batch, _result = POINTER(HaldaBatchC), POINTER(HaldaResultC)
_model, _fleets, _out = POINTER(HaldaModelC), POINTER(HaldaFleetsC), POINTER(HaldaFleetResultC)
_items, _plans, _plan_out = POINTER(HaldaSubfleetsC), POINTER(HaldaPlansC), POINTER(HaldaPlanResultC)
_table = [_vp, _model, _fleets]  # ctx, model, fleets
_ks = [_vp, c_int32]             # ks (host memory), n_k


def _with_host(name, *args):
    """A device entry, whose last argument is the stream, and its synchronous _host form without it."""
    return {name: (c_int, [*args, _vp]), name + "_host": (c_int, list(args))}


def _knob(family):
    """halda_set_<family>_path(ctx, path) and halda_last_<family>_route(ctx, &route)."""
    return {f"halda_last_{family}_route": (c_int, [_vp, _ip]), f"halda_set_{family}_path": (c_int, [_vp, c_int])}


# name -> (restype, argtypes) of every function include/halda.h declares, in header order (a _host form next to
# its device form)
PROTOTYPES = {
    "halda_version": (c_int, []),
    "halda_init": (c_int, [c_int, _vpp]),
    "halda_solve_batch": (c_int, [_vp, _batch, _result]),
    "halda_solve_batch_device": (c_int, [_vp, _batch, _result, _vp]),
    "halda_solve_batch_device_settled": (c_int, [_vp, _batch, _result, _vp, _vp]),
    "halda_last_kernel_ms": (c_int, [_vp, _dp]),
    "halda_last_solve_kernel_ms": (c_int, [_vp, _dp]),
    "halda_set_timing": (c_int, [_vp, c_int]),
    "halda_last_phase_ms": (c_int, [_vp, _dp]),
    **_with_host("halda_solve_fleets", *_table, *_ks, _out),
    "halda_fleets_plan_create": (c_int, [*_table, *_ks, _out, _vpp]),
    "halda_fleets_plan_launch": (c_int, [_vp, _vp]),
    "halda_fleets_plan_launch_many": (c_int, [_vpp, c_int32, _vpp, c_int32, c_int64, c_int32]),
    "halda_fleets_plan_free": (None, [_vp]),
    "halda_fleets_group_create": (c_int, [_vpp, c_int32, _vpp, POINTER(c_int32)]),
    "halda_fleets_group_launch": (c_int, [_vp, c_int64, c_int32, _vp]),
    "halda_fleets_group_free": (None, [_vp]),
    "halda_set_fleets_path": (c_int, [_vp, c_int]),
    "halda_last_fleet_ms": (c_int, [_vp, _dp]),
    **_with_host("halda_solve_subfleets", *_table, _items, *_ks, _out),
    **_knob("subfleets"),
    **_with_host("halda_solve_variants", _vp, _model, c_int32, _fleets, *_ks, _out),
    **_knob("variants"),
    **_with_host("halda_eval_plans", *_table, _plans, _plan_out),
    **_with_host("halda_solve_fleets_plans", *_table, *_ks, _plans, _plan_out, _out),
    **_knob("plans"),
    **_with_host("halda_solve_fleets_bounded", *_table, *_ks, POINTER(HaldaBoundsC), _out),
    **_knob("bounds"),
    **_with_host("halda_solve_fleets_boxed", *_table, *_ks, POINTER(HaldaBoxC), _out),
    **_with_host("halda_solve_fleets_budget", *_table, c_int32, POINTER(HaldaBudgetC), POINTER(HaldaFrontierC)),
    "halda_budget_lds_bytes": (c_int64, [c_int32] * 3),
    **_with_host("halda_solve_change", *_table, _items, c_int32, POINTER(HaldaChangeC), POINTER(HaldaChangeFrontierC)),
    "halda_change_lds_bytes": (c_int64, [c_int32] * 4),
    **_with_host("halda_solve_subsets", *_table, POINTER(HaldaSubsetsC), *_ks, POINTER(HaldaSubsetFrontierC)),
    "halda_subsets_count": (c_int64, [c_int32, c_int32]),
    **_knob("subsets"),
    **_with_host("halda_solve_change_subsets", *_table, c_int32, POINTER(HaldaChangeSubsetsC),
                 POINTER(HaldaChangeSubsetFrontierC)),
    "halda_change_subsets_max_deficit": (c_int64, [_vp, c_int32, c_uint64, c_int32, c_int32]),
    "halda_change_subsets_launch_bytes": (c_int64, [c_int32, c_int32, c_int64]),
    "halda_set_change_subsets_chunk": (c_int, [_vp, c_int64]),
    "halda_resident_release": (c_int, [_vp]),
    "halda_host_alloc": (c_int, [c_size_t, _vpp]),
    "halda_host_free": (None, [_vp]),
    "halda_init_multi": (c_int, [c_int, _vp, _vpp]),
    "halda_solve_fleets_multi": (c_int, [*_table, *_ks, _out]),
    "halda_free_multi": (None, [_vp]),
    "halda_comm_unique_id": (c_int, [_vp]),
    "halda_comm_init": (c_int, [_vpp, c_int, c_int, c_char_p, c_int]),
    "halda_comm_destroy": (None, [_vp]),
    "halda_solve_fleets_sharded": (c_int, [_vp, _vp, _model, _fleets, *_ks, _out, _vp]),
    "halda_solve_fleets_sharded_emulated": (c_int, [_vp, c_int32, c_int32, _model, _fleets, *_ks, _out, _vp]),
    "halda_last_lowered": (c_int, [_vp, _batch, _result]),
    "halda_lds_bytes": (c_int64, [c_int32] * 4),
    "halda_last_error": (c_int, [c_char_p, c_size_t]),
    "halda_free": (None, [_vp]),
}

EXPORTS = tuple(PROTOTYPES)

# include/halda_boxes.h, the companion header of the many-boxes entry: its struct and prototypes, declared here
# once like halda.h's and applied by load_library with them (tests/test_boxes.py holds them to that header)
BOXES_STRUCTS = {HaldaBoxesC: "halda_boxes"}
BOXES_PROTOTYPES = {
    **_with_host("halda_solve_fleets_boxes", *_table, *_ks, POINTER(HaldaBoxesC), _out),
    **_knob("boxes"),
}
