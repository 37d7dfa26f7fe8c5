"""Exact selection under boxes without a GPU: the exported surface, the Python argument and gate errors, raised
before any packing or library call, the gathering of a box onto a kept list, and the assembly of the [box][d]
frontier with a stubbed solve."""

import ctypes
import math
from types import SimpleNamespace

import pytest

from distilp_amd.solver import _abi
from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import halda_select_devices_exact, halda_subset_frontier, halda_subset_frontier_boxes
from distilp_amd.solver import subsets_bounded as sx

from . import bounds_cases as bc

NEW = ("halda_solve_subsets_boxed", "halda_solve_subsets_boxed_host", "halda_last_subsets_boxed_route",
       "halda_set_subsets_boxed_path", "halda_set_subsets_boxed_chunk")


def test_the_library_and_the_packages_export_the_new_surface():
    assert sorted(_abi.SUBSETS_BOXED_PROTOTYPES) == sorted(NEW)
    assert lh.ROUTES["subsets_boxed"] == ("none", "register", "expand", "tables", "mixed")
    raw, lib = ctypes.CDLL(str(lh.LIB_PATH)), lh.load_library(lh.LIB_PATH)
    assert all(hasattr(raw, name) for name in NEW) and lib.halda_version() == 3
    assert lib.halda_set_subsets_boxed_path(None, 1) == -22 and lib.halda_set_subsets_boxed_chunk(None, 0) == -22
    import distilp.solver as alias

    assert alias.halda_subset_frontier_boxes is halda_subset_frontier_boxes


def no_call(*a, **k):
    raise AssertionError("packed or reached the library")


BOX4 = (None, [5, 5, 5, 5])
BAD_CALLS = [
    # (boxes, max_drop, keep, exception, text)
    ([], None, None, ValueError, "empty"),
    (7, None, None, ValueError, "not a sequence"),
    ([(None, [5, 5, 5])], None, None, ValueError, "3 entries"),
    ([([0, 1, 1, 1], None)], None, None, ValueError, ">= 1"),
    ([BOX4], 4, None, ValueError, "max_drop = 4 is beyond"),
    ([BOX4], 2, [0, 1, 2], ValueError, "max_drop = 2 is beyond"),
    ([BOX4], -1, None, ValueError, ">= 0"),
    ([BOX4], None, [4], IndexError, "device index 4"),
]


@pytest.mark.parametrize("boxes,max_drop,keep,exc,text", BAD_CALLS)
def test_argument_errors_come_before_any_packing(monkeypatch, llama_online_model, boxes, max_drop, keep, exc, text):
    monkeypatch.setattr(sx, "fleet_table", no_call)
    monkeypatch.setattr(sx, "get_context", no_call)
    with pytest.raises(exc, match=text):
        halda_subset_frontier_boxes(list(bc.devices(4, 0)), llama_online_model, boxes, max_drop, keep)


def test_the_bounds_keyword_checks_box_route_and_gate_first(monkeypatch, llama_online_model):
    monkeypatch.setattr(sx, "fleet_table", no_call)
    devs, model = list(bc.devices(4, 0)), llama_online_model
    for fn in (halda_subset_frontier, halda_select_devices_exact):
        with pytest.raises(ValueError, match="3 entries"):
            fn(devs, model, bounds=(None, [5, 5, 5]))
        with pytest.raises(ValueError, match="wave route only"):
            fn(devs, model, bounds=BOX4, route="wide")
        with pytest.raises(ValueError, match="max_drop = 9 is beyond"):
            fn(devs, model, 9, bounds=BOX4)
    with pytest.raises(ValueError, match="at most 64 devices"):
        halda_subset_frontier(list(bc.devices(4, 0)) * 17, model, bounds=(None, [5] * 68))


def test_a_box_is_gathered_by_parent_index():
    box = (None, [10, 11, 12, 13, 14], [0, 1, 2, 3, 4], None)
    assert sx.gather_bounds(box, [4, 0, 2]) == (None, [14, 10, 12], [4, 0, 2], None)
    assert sx.gather_bounds(None, [1]) is None and sx.gather_bounds(([1, 2], [3, 4]), [1]) == ([2], [4])


def test_the_frontier_is_assembled_per_box_with_the_strict_earliest_minimum(llama_online_model):
    """A stubbed solve prices item (f, kept, b) from the kept list and the box alone: under box 1 device 2 may not
    be kept; equal values leave the earliest candidate."""
    seen = []

    def solve(items):
        seen.extend(items)
        return [None if b == 1 and 2 in kept else SimpleNamespace(obj_value=float(len(kept) + (0 in kept)))
                for _, kept, b in items]

    rows = halda_subset_frontier_boxes(list(bc.devices(4, 0)), llama_online_model, [None, BOX4], 2, [3], _solve_items=solve)
    assert len(rows) == 2 and [len(r) for r in rows] == [3, 3] and {b for _, _, b in seen} == {0, 1}
    assert all(0 <= i < 4 for _, kept, _ in seen for i in kept) and all(3 in kept for _, kept, _ in seen)
    assert [(p.dropped, p.kept, p.obj_value) for p in rows[0]] == [([], [0, 1, 2, 3], 5.0), ([0], [1, 2, 3], 3.0),
                                                                   ([0, 1], [2, 3], 2.0)]
    assert rows[1][0].result is None and rows[1][0].obj_value == math.inf and rows[1][0].kept == []
    assert [(p.dropped, p.obj_value) for p in rows[1][1:]] == [([2], 4.0), ([0, 2], 2.0)]
    kept, r = halda_select_devices_exact(list(bc.devices(4, 0)), llama_online_model, 2, [3], bounds=BOX4,
                                         _solve_lists=lambda ls: [SimpleNamespace(obj_value=float(len(k))) for k in ls])
    assert kept == [2, 3] and r.obj_value == 2.0
