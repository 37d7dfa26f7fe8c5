"""The C ABI of libhalda (include/halda.h, and include/halda_boxes.h beside it) as ctypes declarations: every
struct, in header order, and the prototype of every function. `_libhalda.load_library` applies PROTOTYPES,
BOXES_PROTOTYPES, BOXES_WIDE_PROTOTYPES (include/halda_boxes_wide.h), WIDE_PROTOTYPES (include/halda_wide.h) PARTITION_PROTOTYPES (include/halda_partition.h) and PARTITION_CLASSES_PROTOTYPES
(include/halda_partition_classes.h) to the library it opens, so no call can reach a function with ctypes' default `int` arguments
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

# include/halda_subfleets_boxed.h, the companion header of sub-fleets under boxes: halda_boxes' fields and the
# items' box indices; applied by load_library with the others (tests/test_subfleets_bounded.py holds them to
# that header)
class HaldaSubBoxesC(ctypes.Structure):
    _fields_ = [("n_box", c_int32)] + _ptrs("w_min", "w_max", "n_min", "n_max", "item_box")


SUBBOX_STRUCTS = {HaldaSubBoxesC: "halda_sub_boxes"}
SUBBOX_PROTOTYPES = {
    **_with_host("halda_solve_subfleets_boxed", *_table, _items, *_ks, POINTER(HaldaSubBoxesC), _out),
    **_knob("subfleets_boxed"),
}

# include/halda_subsets_boxed.h, the companion header of exact selection under boxes (it takes halda.h's
# halda_subsets / halda_subset_frontier and halda_boxes.h's halda_boxes): its prototypes, applied by load_library
# with the others (tests/test_subsets_bounded.py holds them to that header)
SUBSETS_BOXED_PROTOTYPES = {
    **_with_host("halda_solve_subsets_boxed", *_table, POINTER(HaldaSubsetsC), *_ks, POINTER(HaldaBoxesC),
                 POINTER(HaldaSubsetFrontierC)),
    **_knob("subsets_boxed"),
    "halda_set_subsets_boxed_chunk": (c_int, [_vp, c_int64]),
}

# include/halda_boxes_wide.h, the companion header of the workgroup route of the many-boxes entry (it takes
# halda_boxes.h's struct): its prototypes, applied by load_library with the others (tests/test_boxes_wide.py holds
# them to that header)
BOXES_WIDE_PROTOTYPES = {
    **_with_host("halda_solve_fleets_boxes_wide", *_table, *_ks, POINTER(HaldaBoxesC), _out),
    "halda_boxes_wide_bytes": (c_int, [c_int32] * 3 + [POINTER(c_int64)] * 2),
}

# include/halda_wide.h, the companion header of the workgroup routes of the move budget and the change frontier
# (which take halda.h's structs) and of the rank routes of selection and scale-in / scale-out, whose structs
# follow; its prototypes are applied by load_library with the others
class HaldaSubsetsWideC(ctypes.Structure):
    _fields_ = [("max_drop", c_int32)] + _ptrs("keep_mask")


class HaldaSubsetFrontierWideC(ctypes.Structure):
    _fields_ = _ptrs("status", "obj", "dropped", "best_k")


class HaldaChangeSubsetsWideC(ctypes.Structure):
    _fields_ = (_ptrs("w0", "w_min", "w_max") + [("min_drop", c_int32), ("max_drop", c_int32), ("max_p", c_int32)]
                + _ptrs("keep_mask"))


class HaldaChangeSubsetFrontierWideC(ctypes.Structure):
    _fields_ = _ptrs("status", "obj", "dropped", "loaded", "released", "w", "n")


WIDE_STRUCTS = {HaldaSubsetsWideC: "halda_subsets_wide", HaldaSubsetFrontierWideC: "halda_subset_frontier_wide",
                HaldaChangeSubsetsWideC: "halda_change_subsets_wide",
                HaldaChangeSubsetFrontierWideC: "halda_change_subset_frontier_wide"}
WIDE_PROTOTYPES = {
    **_with_host("halda_solve_fleets_budget_wide", *_table, c_int32, POINTER(HaldaBudgetC), POINTER(HaldaFrontierC)),
    "halda_budget_wide_bytes": (c_int, [c_int32] * 3 + [POINTER(c_int64)] * 2),
    **_with_host("halda_solve_change_wide", *_table, _items, c_int32, POINTER(HaldaChangeC),
                 POINTER(HaldaChangeFrontierC)),
    "halda_change_wide_bytes": (c_int, [c_int32] * 4 + [POINTER(c_int64)] * 2),
    **_with_host("halda_solve_subsets_wide", *_table, POINTER(HaldaSubsetsWideC), *_ks,
                 POINTER(HaldaSubsetFrontierWideC)),
    **_with_host("halda_solve_change_subsets_wide", *_table, c_int32, POINTER(HaldaChangeSubsetsWideC),
                 POINTER(HaldaChangeSubsetFrontierWideC)),
    "halda_change_subsets_wide_launch_bytes": (c_int64, [c_int32] * 4 + [c_int64]),
}

# include/halda_partition.h, the companion header of exact replica partitioning: its structs and prototypes,
# applied by load_library with the others (tests/test_partition.py holds them to that header)
class HaldaPartitionC(ctypes.Structure):
    _fields_ = [("max_groups", c_int32), ("criterion", c_int32)]


class HaldaPartitionFrontierC(ctypes.Structure):
    _fields_ = _ptrs("status", "value", "group_mask", "group_obj", "group_k")


PARTITION_STRUCTS = {HaldaPartitionC: "halda_partition", HaldaPartitionFrontierC: "halda_partition_frontier"}
PARTITION_PROTOTYPES = {
    **_with_host("halda_solve_partition", *_table, POINTER(HaldaPartitionC), *_ks, POINTER(HaldaPartitionFrontierC)),
    "halda_partition_bytes": (c_int64, [c_int32, c_int32]),
}

# include/halda_partition_classes.h, partitioning by device class: its structs and prototypes, applied by
# load_library with the others (tests/test_partition_classes.py holds them to that header)
class HaldaPartitionClassesC(ctypes.Structure):
    _fields_ = [("max_groups", c_int32), ("criterion", c_int32)] + _ptrs("cls", "dev_off")


class HaldaPartitionClassesFrontierC(ctypes.Structure):
    _fields_ = _ptrs("status", "value", "group_code", "group_obj", "group_k")


PARTITION_CLASSES_STRUCTS = {HaldaPartitionClassesC: "halda_partition_classes",
                             HaldaPartitionClassesFrontierC: "halda_partition_classes_frontier"}
PARTITION_CLASSES_PROTOTYPES = {
    **_with_host("halda_solve_partition_classes", *_table, POINTER(HaldaPartitionClassesC), *_ks,
                 POINTER(HaldaPartitionClassesFrontierC)),
    "halda_partition_classes_bytes": (c_int64, [_vp, c_int32, c_int32]),
}
