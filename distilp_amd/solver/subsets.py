"""Exact device selection: the best sub-fleet over ALL subsets of the droppable devices (libhalda
`halda_solve_subsets`).

The reference forces w_i >= 1 on every listed device, so "which of my machines should I use at all?" is a
question about sub-fleets. A candidate is the fleet without d of its droppable devices (every device not in
`keep`), the kept devices in their order; its value is exactly what `halda_solve_subfleets` returns for that
list. Candidates are enumerated by d ascending and, within one d, by their ascending dropped-index lists in
lexicographic order (`itertools.combinations`' order); among equal objectives the earliest wins.

The GPU forms every candidate itself from one 64-bit combo per candidate (bit r: drop the r-th droppable
device) and keeps, per fleet and d, the arg-min on the device: only the frontier -- one point per d --
crosses PCIe. The device orders candidates by the objective it forms; each winner's HALDAResult is then
built by ONE follow-up `halda_solve_subfleets` call over the winning lists, so a point's `result` is that
entry's, bit for bit, and the selection takes the running minimum over d again on these host-formed
obj_values (as budget.py does for its frontier).
"""

from __future__ import annotations

import ctypes
import itertools
import math
import numbers
from dataclasses import dataclass
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._abi import HaldaSubsetFrontierC, HaldaSubsetsC
from ._libhalda import STATUS_OPTIMAL, get_context, last_route, ptr, set_path
from .coefficients import HALDAResult
from .fleets import DEV_HEAD, _host_struct, fleet_table, model_struct
from .fleets import _bind as _bind_subsets  # noqa: F401 -- the identity, for callers from before load_library bound all
from .halda import _batch_k_list, _positive_ks
from .lower import kv_bits_to_factor
from .subfleets import check_item_heads, halda_solve_subfleets

MAX_DEVICES = 64  # a candidate is a 64-bit mask; lane = device in the fused kernel
SUBSETS_MAX = 1 << 20  # include/halda.h HALDA_SUBSETS_MAX: candidates per fleet

SolveLists = Callable[[List[List[int]]], List[Optional[HALDAResult]]]


def set_subsets_path(ctx, path: int) -> None:
    """halda_set_subsets_path on a HaldaContext: 0 automatic (default), 1 always expand (test path)."""
    set_path(ctx, "subsets", path)


def last_subsets_route(ctx) -> str:
    """The routes of the context's last halda_solve_subsets call: "fused", "expand", "mixed" or "none"."""
    return last_route(ctx, "subsets")


# ---------------------------------------------------------------- enumeration
def subsets_count(q: int, max_drop: int) -> int:
    """sum over d <= max_drop of C(q, d): the candidates of a fleet with q droppable devices
    (halda_subsets_count, unsaturated)."""
    return sum(math.comb(q, d) for d in range(0, min(max_drop, q) + 1))


def combo_list(q: int, d: int) -> List[int]:
    """The combos of d of q slots in enumeration order (bit r: slot r dropped): ascending index lists,
    lexicographic -- the list the library uploads per (q, d)."""
    return [sum(1 << r for r in c) for c in itertools.combinations(range(q), d)]


def droppable(M: int, keep: Optional[Iterable[int]]) -> List[int]:
    """Slot -> device: the devices of a fleet of M that are not in `keep`, ascending. IndexError for a keep
    index outside the fleet."""
    kept = set()
    for i in (keep or ()):
        if isinstance(i, bool) or not isinstance(i, numbers.Integral) or not 0 <= i < M:
            raise IndexError(f"keep: device index {i!r} out of range for a fleet of {M} devices")
        kept.add(int(i))
    return [i for i in range(M) if i not in kept]


def combo_devices(slots: Sequence[int], combo: int) -> List[int]:
    """The devices a combo drops, ascending."""
    return [slots[r] for r in range(len(slots)) if (combo >> r) & 1]


def candidate_lists(M: int, slots: Sequence[int], d: int) -> Iterable[Tuple[List[int], List[int]]]:
    """(dropped, kept) of every candidate with d devices dropped, in enumeration order."""
    for c in itertools.combinations(slots, d):
        gone = set(c)
        yield list(c), [i for i in range(M) if i not in gone]


def check_max_drop(max_drop, limit: int) -> int:
    """max_drop (None: `limit`) as an int in 0 .. limit; ValueError otherwise."""
    if max_drop is None:
        return limit
    if isinstance(max_drop, bool) or not isinstance(max_drop, numbers.Integral):
        raise ValueError(f"max_drop: {max_drop!r} is not an integer")
    if max_drop < 0:
        raise ValueError("max_drop must be >= 0")
    if max_drop > limit:
        raise ValueError(f"max_drop = {max_drop} is beyond min(droppable devices, M - 1) = {limit}")
    return int(max_drop)


def check_count(q: int, D: int) -> None:
    n = subsets_count(q, D)
    if n > SUBSETS_MAX:
        raise ValueError(f"{n} candidate sub-fleets ({q} droppable devices, up to {D} dropped) exceed the limit of "
                         f"{SUBSETS_MAX}: lower max_drop or keep more devices")


@dataclass(frozen=True)
class SubsetPoint:
    """Point d of a selection frontier: the best candidate with exactly d devices dropped -- the dropped and
    kept device indices (ascending), the HALDAResult of the kept list (indexed within it) and its obj_value.
    Where no candidate with d drops is feasible: dropped = kept = [], result None, obj_value inf."""

    dropped: List[int]
    kept: List[int]
    result: Optional[HALDAResult]
    obj_value: float


_NO_POINT = SubsetPoint([], [], None, math.inf)


def possible_heads(flags: np.ndarray, slots: Sequence[int], D: int) -> List[int]:
    """The devices that are kappa's head in SOME candidate with at most D drops: an is_head device once every
    is_head device in front of it is dropped, any other once all is_head devices and every device in front
    of it are."""
    M, can = len(flags), set(slots)
    heads = [i for i in range(M) if flags[i] & DEV_HEAD]
    out = []
    for i in range(M):
        gone = [h for h in heads if h < i] if i in heads else sorted(set(heads) | set(range(i)))
        if len(gone) <= min(D, M - 1) and all(j in can for j in gone):
            out.append(i)
    return out


def _frontier_by_lists(M: int, slots: Sequence[int], D: int, solve: SolveLists) -> List[SubsetPoint]:
    """The frontier by enumeration: every candidate through `solve`, the strict earliest arg-min per d (the
    specification of the device's pick; the tests' route without a GPU)."""
    pts = []
    for d in range(D + 1):
        cands = list(candidate_lists(M, slots, d))
        res = solve([k for _, k in cands])
        best = None
        for (gone, kept), r in zip(cands, res):
            if r is not None and (best is None or r.obj_value < best.obj_value):  # strict: the earliest stays
                best = SubsetPoint(gone, kept, r, r.obj_value)
        pts.append(best or _NO_POINT)
    return pts


def solve_subsets_table(table, model: ModelProfile, pos: List[int], kv_factor: float, max_drop: int,
                        keep_masks: Optional[np.ndarray], device: int = 0):
    """One halda_solve_subsets_host call on a packed table: (status, obj, dropped_mask, best_k), each
    [n_fleets, max_drop + 1]. obj is the GPU-formed objective."""
    ctx = get_context(device)
    nf, P1 = table.n_fleets, int(max_drop) + 1
    status, obj = np.zeros((nf, P1), np.int32), np.zeros((nf, P1))
    mask, best_k = np.zeros((nf, P1), np.uint64), np.zeros((nf, P1), np.int32)
    fs, hold = _host_struct(table)
    km = None if keep_masks is None else np.ascontiguousarray(keep_masks, np.uint64)
    sub = HaldaSubsetsC(int(max_drop), ptr(km))
    fr = HaldaSubsetFrontierC(ptr(status), ptr(obj), ptr(mask), ptr(best_k))
    karr = np.asarray(pos, np.int32)
    m = model_struct(model, kv_factor)
    ctx.call("halda_solve_subsets_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(sub),
             karr.ctypes.data, len(pos), ctypes.byref(fr))
    del hold
    return status, obj, mask, best_k


def halda_subset_frontier_batch(
    fleets: Sequence[Sequence[DeviceProfile]],
    model: ModelProfile,
    max_drop: Optional[int] = None,
    keep: Optional[Sequence[Optional[Iterable[int]]]] = None,
    k_candidates: Optional[Iterable[int]] = None,
    mip_gap: Optional[float] = 1e-4,
    kv_bits: str = "8bit",
    device: int = 0,
    _solve_lists: Optional[Callable[[int, List[List[int]]], List[Optional[HALDAResult]]]] = None,
) -> List[List[SubsetPoint]]:
    """Per fleet its selection frontier: one SubsetPoint per d = 0 .. min(max_drop, q, M - 1), q the fleet's
    droppable devices (max_drop None: every d the fleet admits -- with nothing kept, every non-empty
    subset). One fleet table and one selection call for all fleets (mixed sizes allowed), then one
    halda_solve_subfleets call over the winning lists. `keep`: per fleet the indices that may not be dropped,
    or None. ValueError before any GPU work for a fleet of more than 64 devices, a max_drop that is negative,
    non-integer or beyond what every fleet admits, or more than 2^20 candidates in a fleet; IndexError for a
    keep index out of range or an empty fleet. `_solve_lists(f, lists)` (tests): the solve of index lists of
    fleet f, in place of the GPU."""
    fleets = [list(d) for d in fleets]
    if keep is not None and len(keep) != len(fleets):
        raise ValueError(f"{len(keep)} keep entries for {len(fleets)} fleets")
    slots, lim = [], []
    for f, devs in enumerate(fleets):
        if not devs:
            raise IndexError("list index out of range")  # the reference's kappa on an empty fleet
        if len(devs) > MAX_DEVICES:
            raise ValueError(f"exact selection needs fleets of at most {MAX_DEVICES} devices, fleet {f} has "
                             f"{len(devs)}")
        slots.append(droppable(len(devs), None if keep is None else keep[f]))
        lim.append(min(len(slots[f]), len(devs) - 1))
    if not fleets:
        return []
    D = check_max_drop(max_drop, max(lim))
    Df = [min(D, x) for x in lim]
    for f in range(len(fleets)):
        check_count(len(slots[f]), Df[f])
    if _solve_lists is not None:
        return [_frontier_by_lists(len(fleets[f]), slots[f], Df[f], lambda ls, f=f: _solve_lists(f, ls))
                for f in range(len(fleets))]
    Ks = _batch_k_list(model, k_candidates)  # halda_solve_batch's k list and k rules
    kv_factor = kv_bits_to_factor(kv_bits)
    pos = _positive_ks(Ks)
    table = fleet_table(fleets, model, _reuse=True)
    if not pos:
        return [[_NO_POINT] * (Df[f] + 1) for f in range(len(fleets))]
    # the packer's error that depends on kappa's head, for every head a candidate can have
    par, hd = [], []
    for f in range(len(fleets)):
        o = int(table.dev_off[f])
        for i in possible_heads(table.flags[o:o + len(fleets[f])], slots[f], Df[f]):
            par.append(f)
            hd.append(o + i)
    check_item_heads(fleets, table, np.asarray(par, np.int64), np.asarray(hd, np.int64), model)
    masks = None
    if keep is not None and any(len(slots[f]) < len(fleets[f]) for f in range(len(fleets))):
        masks = np.asarray([sum(1 << i for i in range(len(fleets[f])) if i not in set(slots[f]))
                            for f in range(len(fleets))], np.uint64)
    status, _, dmask, _ = solve_subsets_table(table, model, pos, kv_factor, D, masks, device)
    items, at = [], {}
    for f in range(len(fleets)):
        for d in range(Df[f] + 1):
            if int(status[f, d]) == STATUS_OPTIMAL:
                m = int(dmask[f, d])
                at[(f, d)] = len(items)
                items.append((f, [i for i in range(len(fleets[f])) if not (m >> i) & 1]))
    res = halda_solve_subfleets(fleets, model, items, k_candidates, mip_gap, kv_bits, device) if items else []
    out = []
    for f in range(len(fleets)):
        pts = []
        for d in range(Df[f] + 1):
            j = at.get((f, d))
            r = None if j is None else res[j]
            if r is None:
                pts.append(_NO_POINT)
                continue
            kept = list(items[j][1])
            gone = set(kept)
            pts.append(SubsetPoint([i for i in range(len(fleets[f])) if i not in gone], kept, r, r.obj_value))
        out.append(pts)
    return out


def halda_subset_frontier(
    devs: Sequence[DeviceProfile],
    model: ModelProfile,
    max_drop: Optional[int] = None,
    keep: Optional[Iterable[int]] = None,
    k_candidates: Optional[Iterable[int]] = None,
    mip_gap: Optional[float] = 1e-4,
    kv_bits: str = "8bit",
    device: int = 0,
    _solve_lists: Optional[SolveLists] = None,
) -> List[SubsetPoint]:
    """The selection frontier of one fleet: point d is the best sub-fleet with exactly d of the droppable
    devices (all but `keep`) left out, d = 0 .. max_drop (None: min(q, M - 1), every candidate there is).
    Point 0 is the full fleet. Each point's `result` equals
    `halda_solve_subfleets([devs], model, [(0, kept)])[0]` bit for bit. ValueError for max_drop beyond
    min(q, M - 1); otherwise the errors of halda_subset_frontier_batch."""
    devs = list(devs)
    if not devs:
        raise IndexError("list index out of range")
    if len(devs) <= MAX_DEVICES:
        check_max_drop(max_drop, min(len(droppable(len(devs), keep)), len(devs) - 1))
    hook = None if _solve_lists is None else (lambda f, ls: _solve_lists(ls))
    return halda_subset_frontier_batch([devs], model, max_drop, None if keep is None else [keep], k_candidates,
                                       mip_gap, kv_bits, device, hook)[0]


def select_point(points: Sequence[SubsetPoint]) -> Optional[SubsetPoint]:
    """The strict, ascending prefix-minimum over d on the host-formed obj_value: among equal objectives the
    fewest drops win. None when no point has a plan."""
    best = None
    for p in points:
        if p.result is not None and (best is None or p.obj_value < best.obj_value):
            best = p
    return best


def halda_select_devices_exact(
    devs: Sequence[DeviceProfile],
    model: ModelProfile,
    max_drop: Optional[int] = None,
    keep: Optional[Iterable[int]] = None,
    k_candidates: Optional[Iterable[int]] = None,
    mip_gap: Optional[float] = 1e-4,
    kv_bits: str = "8bit",
    device: int = 0,
    _solve_lists: Optional[SolveLists] = None,
) -> Tuple[List[int], HALDAResult]:
    """Which devices to use: the optimum over every sub-fleet that leaves out at most max_drop of the
    droppable devices (None: over all of them), not halda_select_devices' greedy walk. Returns (kept
    indices into `devs`, ascending; the HALDAResult of that sub-fleet, indexed within the kept list).
    RuntimeError when no sub-fleet is feasible."""
    best = select_point(halda_subset_frontier(devs, model, max_drop, keep, k_candidates, mip_gap, kv_bits, device,
                                              _solve_lists))
    if best is None:
        raise RuntimeError("No feasible MILP found for any k this round.")
    return list(best.kept), best.result
