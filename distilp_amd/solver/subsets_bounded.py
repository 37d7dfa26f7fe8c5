"""Exact device selection under layer bounds (libhalda `halda_solve_subsets_boxed`).

`halda_subset_frontier` answers "which of my machines should I use at all?" over ALL subsets of the droppable
devices; `halda_solve_subfleets_bounded` prices one sub-fleet inside caps, pins, disabled GPU shares and move
boxes. This is both at once: the candidates, their order, `keep` and the tie rule are subsets.py's, and a
candidate's value under box b is what `halda_solve_subfleets_bounded` returns for (fleet, kept list, b) -- a kept
device stays under the box entry of its PARENT index, a dropped device's entry does not apply, and a device to pin
AND keep goes in `keep`. The boxes travel as the planes `boxes.box_planes` writes in the parents' layout; the GPU
forms every candidate under every box and keeps the arg-min per (box, fleet, d), so only the frontier crosses
PCIe. Each winner's HALDAResult is then built by ONE follow-up `halda_solve_subfleets_bounded` call over the
winning (list, box) items, and the selection takes the running minimum over d again on those host-formed
obj_values, as subsets.py does. Fleets of at most 64 devices (the wave route); the rank route of subsets.py
(route="wide") is not offered under bounds.
"""

from __future__ import annotations

import ctypes
from typing import Callable, Iterable, List, Optional, Sequence

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._abi import HaldaBoxesC, HaldaSubsetFrontierC, HaldaSubsetsC
from ._libhalda import STATUS_OPTIMAL, get_context, last_route, ptr, set_path
from .bounds import Bounds
from .boxes import box_planes, check_boxes
from .coefficients import HALDAResult
from .fleets import _host_struct, fleet_table, model_struct
from .halda import _batch_k_list, _positive_ks
from .lower import kv_bits_to_factor
from .subfleets_bounded import halda_solve_subfleets_bounded
from .subsets import (_NO_POINT, SubsetPoint, candidate_lists, check_candidate_heads, keep_mask_array, selection_gate)

SolveItems = Callable[[List[tuple]], List[Optional[HALDAResult]]]


def set_subsets_boxed_path(ctx, path: int) -> None:
    """halda_set_subsets_boxed_path on a HaldaContext: 0 automatic (default), 1 always expand (test path)."""
    set_path(ctx, "subsets_boxed", path)


def set_subsets_boxed_chunk(ctx, items: int) -> None:
    """halda_set_subsets_boxed_chunk on a HaldaContext: the most items of one launch (0: the default, 2^22)."""
    ctx.call("halda_set_subsets_boxed_chunk", ctx.ctx, int(items), lock=False)


def last_subsets_boxed_route(ctx) -> str:
    """The routes of the context's last halda_solve_subsets_boxed call: "register", "tables", "expand", "mixed"
    (they differ by d) or "none"."""
    return last_route(ctx, "subsets_boxed")


def solve_subsets_boxed_table(table, model: ModelProfile, pos: List[int], kv_factor: float, max_drop: int,
                              masks: Optional[np.ndarray], planes, device: int = 0):
    """One halda_solve_subsets_boxed_host call on a packed table: (status, obj, dropped_mask, best_k), each
    [n_box, n_fleets, max_drop + 1]. planes: box_planes' four [n_box, n_devices] arrays (None: no bound on that
    side); obj is the GPU-formed objective."""
    planes = [None if p is None else np.ascontiguousarray(p, np.int32) for p in planes]
    shapes = {p.shape for p in planes if p is not None}
    if len(planes) != 4 or len(shapes) != 1 or next(iter(shapes))[1:] != (table.n_devices,):
        raise ValueError(f"planes: expected (w_min, w_max, n_min, n_max), each None or one [n_box, {table.n_devices}]")
    nb, nf, P1 = int(next(iter(shapes))[0]), table.n_fleets, int(max_drop) + 1
    ctx = get_context(device)
    status, obj = np.zeros((nb, nf, P1), np.int32), np.zeros((nb, nf, P1))
    mask, best_k = np.zeros((nb, nf, P1), np.uint64), np.zeros((nb, nf, P1), np.int32)
    fs, hold = _host_struct(table)
    km = None if masks is None else np.ascontiguousarray(masks, np.uint64)
    sub = HaldaSubsetsC(int(max_drop), ptr(km))
    bx = HaldaBoxesC(nb, *(ptr(p) for p in planes))
    fr = HaldaSubsetFrontierC(ptr(status), ptr(obj), ptr(mask), ptr(best_k))
    karr = np.asarray(pos, np.int32)
    m = model_struct(model, kv_factor)
    ctx.call("halda_solve_subsets_boxed_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(sub),
             karr.ctypes.data, len(pos), ctypes.byref(bx), ctypes.byref(fr))
    del hold
    return status, obj, mask, best_k


def gather_bounds(entry, kept: Sequence[int]):
    """A fleet's bounds entry restricted to the kept devices, in list order (None stays None): what
    halda_solve_bounded_batch takes for the materialised list."""
    return None if entry is None else tuple(None if a is None else [a[j] for j in kept] for a in entry)


def _points_by_items(sizes, slots, Df, nb: int, solve: SolveItems) -> List[List[List[SubsetPoint]]]:
    """The frontier by enumeration: every (candidate, box) through `solve`, the strict earliest arg-min per
    (box, fleet, d) -- the specification of the device's pick, and the tests' route without a GPU."""
    out = [[[] for _ in sizes] for _ in range(nb)]
    for b in range(nb):
        for f, M in enumerate(sizes):
            for d in range(Df[f] + 1):
                cands = list(candidate_lists(M, slots[f], d))
                best = None
                for (gone, kept), r in zip(cands, solve([(f, kept, b) for _, kept in cands])):
                    if r is not None and (best is None or r.obj_value < best.obj_value):  # strict: the earliest stays
                        best = SubsetPoint(gone, kept, r, r.obj_value)
                out[b][f].append(best or _NO_POINT)
    return out


def frontier_boxes_batch(fleets: Sequence[Sequence[DeviceProfile]], model: ModelProfile,
                         boxes: Sequence[Sequence[Bounds]], max_drop: Optional[int] = None,
                         keep: Optional[Sequence[Optional[Iterable[int]]]] = None,
                         k_candidates: Optional[Iterable[int]] = None, kv_bits: str = "8bit", device: int = 0,
                         _solve_items: Optional[SolveItems] = None) -> List[List[List[SubsetPoint]]]:
    """[box][fleet][d] SubsetPoints: per box and fleet the selection frontier of halda_subset_frontier_batch inside
    that box. `boxes[b]` is what halda_solve_boxes_batch takes: one entry per fleet, each None, (w_min, w_max) or
    (w_min, w_max, n_min, n_max) over that fleet's devices. One fleet table and ONE selection call for all boxes
    and fleets, then one halda_solve_subfleets_bounded call over the winning (list, box) items. ValueError before
    any packing for what check_boxes or the subsets gate refuses. `_solve_items(items)` (tests): the solve of
    (f, kept, b) items, in place of the GPU."""
    kv_factor = kv_bits_to_factor(kv_bits)
    fleets = [list(d) for d in fleets]
    sizes = [len(d) for d in fleets]
    checked = check_boxes(boxes, sizes)
    slots, D, Df = selection_gate(fleets, keep, max_drop)
    nb, nf = len(checked), len(fleets)
    if not fleets:
        return [[] for _ in range(nb)]
    if _solve_items is not None:
        return _points_by_items(sizes, slots, Df, nb, _solve_items)
    pos = _positive_ks(_batch_k_list(model, k_candidates))  # halda_solve_batch's k list and k rules
    table = fleet_table(fleets, model, _reuse=True)
    if not pos:
        return [[[_NO_POINT] * (Df[f] + 1) for f in range(nf)] for _ in range(nb)]
    check_candidate_heads(fleets, table, slots, Df, model)
    status, _, dmask, _ = solve_subsets_boxed_table(table, model, pos, kv_factor, D,
                                                    keep_mask_array(fleets, slots, keep),
                                                    box_planes(table, checked, checked=True), device)
    items, at = [], {}
    for b in range(nb):
        for f in range(nf):
            for d in range(Df[f] + 1):
                if int(status[b, f, d]) == STATUS_OPTIMAL:
                    at[(b, f, d)] = len(items)
                    items.append((f, [i for i in range(sizes[f]) if not (int(dmask[b, f, d]) >> i) & 1], b))
    res = halda_solve_subfleets_bounded(fleets, model, items, boxes, k_candidates, kv_bits, device) if items else []
    out = []
    for b in range(nb):
        rows = []
        for f in range(nf):
            pts = []
            for d in range(Df[f] + 1):
                j = at.get((b, f, d))
                r = None if j is None else res[j]
                if r is None:
                    pts.append(_NO_POINT)
                    continue
                kept = list(items[j][1])
                pts.append(SubsetPoint([i for i in range(sizes[f]) if i not in set(kept)], kept, r, r.obj_value))
            rows.append(pts)
        out.append(rows)
    return out


def halda_subset_frontier_boxes(devs: Sequence[DeviceProfile], model: ModelProfile, boxes: Sequence[Bounds],
                                max_drop: Optional[int] = None, keep: Optional[Iterable[int]] = None,
                                k_candidates: Optional[Iterable[int]] = None, kv_bits: str = "8bit", device: int = 0,
                                _solve_items: Optional[SolveItems] = None) -> List[List[SubsetPoint]]:
    """One fleet's selection frontier under each of several boxes, [box][d], from ONE selection call: a cap ladder,
    or "CPU-only on device i" for several i. boxes[b] is the fleet's box b: None, (w_min, w_max) or (w_min, w_max,
    n_min, n_max) over `devs`. Point (b, d) is the best sub-fleet with exactly d of the droppable devices (all but
    `keep`) left out, inside box b restricted to the kept devices; its `result` equals
    halda_solve_subfleets_bounded([devs], model, [(0, kept, b)], [[box] for box in boxes])[0] bit for bit. Fleets of
    at most 64 devices. ValueError before any packing for what check_boxes or halda_subset_frontier's gate refuses;
    IndexError for an empty fleet or a keep index out of range."""
    devs = list(devs)
    if not devs:
        raise IndexError("list index out of range")
    try:
        per_fleet = [[box] for box in boxes]
    except TypeError:
        raise ValueError(f"boxes: {boxes!r} is not a sequence of boxes") from None
    rows = frontier_boxes_batch([devs], model, per_fleet, max_drop, None if keep is None else [keep], k_candidates,
                                kv_bits, device, _solve_items)
    return [r[0] for r in rows]
