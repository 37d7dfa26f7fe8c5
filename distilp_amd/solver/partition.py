"""Exact replica partitioning: one fleet as r = 1 .. R independent pipelines (libhalda `halda_solve_partition`,
include/halda_partition.h).

Should these M machines run as one pipeline, or as two or three replicas, and which machine goes where? A group
is a set of devices; its value val[S] is what `halda_solve_subfleets` gives the list of S's devices in ascending
order. A partition into r groups is priced by its slowest group (criterion "max") or by the sum of its groups'
objectives (criterion "sum", r times the mean). The GPU solves every one of the 2^M - 1 groups and runs the
dynamic programme over subsets

    best_1[S] = val[S];   best_r[S] = min over T, lowbit(S) in T, T a proper subset of S, of
                                      op(val[T], best_{r-1}[S \\ T])

with op = max or +, taking the minimum on the pair (value, T): among equal values the smallest T as an unsigned
integer wins. Only the frontier -- one point per r -- crosses PCIe. Under "max" the groups below the slowest one
are only held at or below it; that tie rule, not the objective, decides them: ask for "sum" where every replica's
speed matters.

Each point's group results are then built by ONE follow-up `halda_solve_subfleets` call over all winning lists,
so a group's HALDAResult is that entry's, bit for bit, and a point's value is formed again on the host from
those obj_values in the recurrence's operand order (as subsets.py re-forms its winners).

By device class (route="classes", libhalda `halda_solve_partition_classes`, include/halda_partition_classes.h):
a fleet of up to 256 devices of at most 8 kinds. Devices whose packed table rows are equal bit for bit form a
class; a group is then how many devices of each class it takes, and the same recurrence runs over count vectors
-- 17^4 = 83,521 groups for 4 kinds x 16 machines, against 2^64 masks. Group g of a point receives, per class,
the next unused devices of that class in ascending index.
"""

from __future__ import annotations

import ctypes
import math
import numbers
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._abi import HaldaPartitionC, HaldaPartitionClassesC, HaldaPartitionClassesFrontierC, HaldaPartitionFrontierC
from ._libhalda import STATUS_OPTIMAL, get_context, load_library, ptr
from .coefficients import HALDAResult
from .fleets import BYTE_FIELDS, DEV_HEAD, F64_FIELDS, _host_struct, fleet_table, model_struct
from .halda import _batch_k_list, _positive_ks
from .lower import kv_bits_to_factor
from .subfleets import check_item_heads, halda_solve_subfleets

MAX_DEVICES = 20  # 2^20 masks per fleet: include/halda.h HALDA_SUBSETS_MAX
MAX_GROUPS = 8
LDS_DEVICES = 13  # fleets up to here: the level kernel reads LDS copies of its two planes
CRITERIA = ("max", "sum")
SLOTS = 8  # group slots per point in halda_partition_frontier
ROUTES = ("masks", "classes", "auto")
# the gate of the class route (include/halda_partition_classes.h)
CLASS_MAX_DEVICES = 256
MAX_CLASSES = 8
MAX_CODES = 1 << 20
MAX_PAIRS = 1 << 32
LDS_CODES = 8192  # every fleet up to here: the class route's level kernel reads LDS copies of its two planes


@dataclass(frozen=True)
class PartitionPoint:
    """Point r of a partition frontier: the best split into exactly r groups -- `groups` the ascending device
    index lists in backtrack order (group 0 holds device 0, group 1 the lowest device not in group 0, ...),
    `results[g]` the HALDAResult of group g (indexed within its list), `value` the slowest group's obj_value
    ("max") or the groups' sum ("sum"). Where no partition into r groups is feasible: groups = results = None,
    value inf."""

    groups: Optional[List[List[int]]]
    results: Optional[List[HALDAResult]]
    value: float


_NO_POINT = PartitionPoint(None, None, math.inf)


def partition_bytes(max_devices: int, max_groups: int) -> int:
    """halda_partition_bytes: the planes of one fleet -- per mask val (8 bytes), k (4), two best planes (16) and
    an arg entry (4) per level r = 2 .. max_groups -- or -1 outside the gate."""
    return int(load_library().halda_partition_bytes(int(max_devices), int(max_groups)))


def check_gate(sizes: Sequence[int], max_groups, criterion) -> int:
    """The gate of halda_solve_partition from the shapes alone: the criterion's code (0 "max", 1 "sum").
    ValueError for an unknown criterion, a max_groups outside 1 .. 8 or beyond every fleet's size, or a fleet
    of more than 20 devices."""
    if criterion not in CRITERIA:
        raise ValueError(f"criterion: {criterion!r} is not one of {CRITERIA}")
    if isinstance(max_groups, bool) or not isinstance(max_groups, numbers.Integral):
        raise ValueError(f"max_groups: {max_groups!r} is not an integer")
    if not 1 <= max_groups <= MAX_GROUPS:
        raise ValueError(f"max_groups must be in 1..{MAX_GROUPS}, got {max_groups}")
    for f, m in enumerate(sizes):
        if m > MAX_DEVICES:
            raise ValueError(f"exact partitioning needs fleets of at most {MAX_DEVICES} devices, fleet {f} has {m}")
    if sizes and max_groups > max(sizes):
        raise ValueError(f"max_groups = {max_groups} is beyond the {max(sizes)} devices of the largest fleet")
    return CRITERIA.index(criterion)


def device_classes(table, f: int):
    """The classes of fleet f of a packed table: (cls, counts, order). Devices whose rows are equal bit for bit in
    every field (flags included) share a class; classes are numbered by first occurrence. cls[i] is device i's
    class, counts[c] the size of class c, order the devices class-major, ascending index within a class."""
    a, b = int(table.dev_off[f]), int(table.dev_off[f + 1])
    rows = np.stack([np.asarray(getattr(table, n)[a:b], np.uint64) for n in ("os_class", "flags")]
                    + [np.ascontiguousarray(getattr(table, n)[a:b], np.float64).view(np.uint64)
                       for n in F64_FIELDS + BYTE_FIELDS], axis=1)
    _, first, inv = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    cls = rank[inv.reshape(-1)].astype(np.int32)
    return cls, np.bincount(cls).astype(np.int32), np.argsort(cls, kind="stable").astype(np.int32)


def check_gate_classes(counts_per_fleet: Sequence[Sequence[int]], max_groups, criterion) -> int:
    """The gate of halda_solve_partition_classes from the class sizes alone: the criterion's code. ValueError for
    an unknown criterion, a max_groups outside 1 .. 8 or beyond every fleet's size, or a fleet of more than 256
    devices, 8 classes, 2^20 codes or 2^32 pair evaluations a level."""
    sizes = [int(sum(int(c) for c in cnt)) for cnt in counts_per_fleet]
    for f, cnt in enumerate(counts_per_fleet):
        if sizes[f] > CLASS_MAX_DEVICES:
            raise ValueError(f"partitioning by class needs fleets of at most {CLASS_MAX_DEVICES} devices, "
                             f"fleet {f} has {sizes[f]}")
        if len(cnt) > MAX_CLASSES:
            raise ValueError(f"partitioning by class needs at most {MAX_CLASSES} classes, fleet {f} has {len(cnt)}")
        codes = math.prod(int(c) + 1 for c in cnt)
        if codes > MAX_CODES:
            raise ValueError(f"partitioning by class needs at most 2^20 codes, fleet {f} has {codes}")
        pairs = math.prod((int(c) + 1) * (int(c) + 2) // 2 for c in cnt)
        if pairs > MAX_PAIRS:
            raise ValueError(f"partitioning by class needs at most 2^32 pair evaluations per level, "
                             f"fleet {f} has {pairs}")
    code = check_gate([], max_groups, criterion)
    if sizes and max_groups > max(sizes):
        raise ValueError(f"max_groups = {max_groups} is beyond the {max(sizes)} devices of the largest fleet")
    return code


def partition_classes_bytes(counts: Sequence[int], max_groups: int) -> int:
    """halda_partition_classes_bytes: the planes of one fleet of these class sizes -- per code val (8 bytes),
    k (4), two best planes (16) and an arg entry (4) per level r = 2 .. max_groups -- or -1 outside the gate."""
    arr = np.asarray(list(counts), np.int32)
    return int(load_library().halda_partition_classes_bytes(arr.ctypes.data, len(arr), int(max_groups)))


def code_counts(code: int, counts: Sequence[int]) -> List[int]:
    """The count vector of a group code: digit c in radix counts[c] + 1, class 0 least significant."""
    out = []
    for c in counts:
        out.append(code % (int(c) + 1))
        code //= int(c) + 1
    return out


def mask_devices(mask: int) -> List[int]:
    """The devices of a group mask, ascending."""
    return [i for i in range(MAX_DEVICES) if (mask >> i) & 1]


def combine(values: Sequence[float], criterion: str) -> float:
    """A point's value from its groups' values in backtrack order, in the recurrence's operand order:
    op(v_0, op(v_1, ... op(v_{r-2}, v_{r-1})))."""
    acc = values[-1]
    for v in reversed(values[:-1]):
        acc = v + acc if criterion == "sum" else max(v, acc)
    return acc


def solve_partition_table(table, model: ModelProfile, pos: List[int], kv_factor: float, max_groups: int,
                          criterion: int, device: int = 0):
    """One halda_solve_partition_host call on a packed table: (status [nf, R], value [nf, R], group_mask,
    group_obj, group_k [nf, R, 8]). value and group_obj are the GPU-formed objectives."""
    ctx = get_context(device)
    nf, R = table.n_fleets, int(max_groups)
    status, value = np.zeros((nf, R), np.int32), np.zeros((nf, R))
    gmask, gobj, gk = np.zeros((nf, R, SLOTS), np.uint32), np.zeros((nf, R, SLOTS)), np.zeros((nf, R, SLOTS), np.int32)
    fs, hold = _host_struct(table)
    part = HaldaPartitionC(R, int(criterion))
    fr = HaldaPartitionFrontierC(ptr(status), ptr(value), ptr(gmask), ptr(gobj), ptr(gk))
    karr = np.asarray(pos, np.int32)
    m = model_struct(model, kv_factor)
    ctx.call("halda_solve_partition_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(part),
             karr.ctypes.data, len(pos), ctypes.byref(fr))
    del hold
    return status, value, gmask, gobj, gk


def solve_partition_classes_table(table, cls: np.ndarray, model: ModelProfile, pos: List[int], kv_factor: float,
                                  max_groups: int, criterion: int, device: int = 0):
    """One halda_solve_partition_classes_host call on a packed table and every device's class id: (status
    [nf, R], value [nf, R], group_code, group_obj, group_k [nf, R, 8])."""
    ctx = get_context(device)
    nf, R = table.n_fleets, int(max_groups)
    status, value = np.zeros((nf, R), np.int32), np.zeros((nf, R))
    gcode, gobj, gk = np.zeros((nf, R, SLOTS), np.uint32), np.zeros((nf, R, SLOTS)), np.zeros((nf, R, SLOTS), np.int32)
    fs, hold = _host_struct(table)
    cls = np.ascontiguousarray(cls, np.int32)
    off = np.ascontiguousarray(table.dev_off, np.int64)
    part = HaldaPartitionClassesC(R, int(criterion), ptr(cls), ptr(off))
    fr = HaldaPartitionClassesFrontierC(ptr(status), ptr(value), ptr(gcode), ptr(gobj), ptr(gk))
    karr = np.asarray(pos, np.int32)
    m = model_struct(model, kv_factor)
    ctx.call("halda_solve_partition_classes_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(part),
             karr.ctypes.data, len(pos), ctypes.byref(fr))
    del hold
    return status, value, gcode, gobj, gk


def _class_groups(codes: Sequence[int], counts: np.ndarray, order: np.ndarray) -> List[List[int]]:
    """The device lists of a point's group codes: group g receives, per class, the next unused devices of that
    class in ascending index, listed in class order."""
    start = np.concatenate([[0], np.cumsum(counts)])
    used = [0] * len(counts)
    out = []
    for code in codes:
        devs = []
        for c, n in enumerate(code_counts(int(code), counts)):
            a = int(start[c]) + used[c]
            devs += [int(i) for i in order[a:a + n]]
            used[c] += n
        out.append(devs)
    return out


def halda_partition_frontier_batch(
    fleets: Sequence[Sequence[DeviceProfile]],
    model: ModelProfile,
    max_groups: int,
    criterion: str = "max",
    k_candidates: Optional[Iterable[int]] = None,
    kv_bits: str = "8bit",
    device: int = 0,
    route: str = "masks",
) -> List[List[PartitionPoint]]:
    """Per fleet its partition frontier: one PartitionPoint per r = 1 .. max_groups (a fleet of fewer than r
    devices has no point r). One fleet table and one partition call for all fleets (mixed sizes allowed), then
    one halda_solve_subfleets call over the winning lists. ValueError before packing for a fleet of more than
    20 devices, a max_groups outside 1 .. 8 or beyond every fleet's size, or an unknown criterion; IndexError
    for an empty fleet. route="classes" partitions by device class (fleets of up to 256 devices of at most 8
    kinds: check_gate_classes); "auto" takes the masks wherever every fleet has at most 20 devices."""
    if route not in ROUTES:
        raise ValueError(f"route: {route!r} is not one of {ROUTES}")
    fleets = [list(d) for d in fleets]
    for devs in fleets:
        if not devs:
            raise IndexError("list index out of range")  # the reference's kappa on an empty fleet
    if route == "auto":
        route = "masks" if all(len(d) <= MAX_DEVICES for d in fleets) else "classes"
    if route == "classes":
        return _frontier_batch_classes(fleets, model, max_groups, criterion, k_candidates, kv_bits, device)
    code = check_gate([len(d) for d in fleets], max_groups, criterion)
    if not fleets:
        return []
    R = int(max_groups)
    Ks = _batch_k_list(model, k_candidates)  # halda_solve_batch's k list and k rules
    kv_factor = kv_bits_to_factor(kv_bits)
    pos = _positive_ks(Ks)
    table = fleet_table(fleets, model, _reuse=True)
    if not pos:
        return [[_NO_POINT] * R for _ in fleets]
    # the packer's error that depends on kappa's head: every device heads some group (the group of it alone)
    par = np.repeat(np.arange(len(fleets), dtype=np.int64), [len(d) for d in fleets])
    check_item_heads(fleets, table, par, np.arange(len(par), dtype=np.int64), model)
    status, _, gmask, _, _ = solve_partition_table(table, model, pos, kv_factor, R, code, device)
    items, at = [], {}
    for f in range(len(fleets)):
        for r in range(1, R + 1):
            if int(status[f, r - 1]) == STATUS_OPTIMAL:
                at[(f, r)] = len(items)
                items += [(f, mask_devices(int(gmask[f, r - 1, g]))) for g in range(r)]
    res = halda_solve_subfleets(fleets, model, items, k_candidates, kv_bits=kv_bits, device=device) if items else []
    out = []
    for f in range(len(fleets)):
        pts = []
        for r in range(1, R + 1):
            j = at.get((f, r))
            rs = None if j is None else res[j:j + r]
            if rs is None or any(x is None for x in rs):
                pts.append(_NO_POINT)
                continue
            pts.append(PartitionPoint([list(items[j + g][1]) for g in range(r)], list(rs),
                                      combine([x.obj_value for x in rs], criterion)))
        out.append(pts)
    return out


def _frontier_batch_classes(fleets, model, max_groups, criterion, k_candidates, kv_bits, device):
    """halda_partition_frontier_batch by device class."""
    check_gate([], max_groups, criterion)  # the errors that need no table
    if not fleets:
        return []
    R = int(max_groups)
    Ks = _batch_k_list(model, k_candidates)
    kv_factor = kv_bits_to_factor(kv_bits)
    pos = _positive_ks(Ks)
    table = fleet_table(fleets, model, _reuse=True)
    classes = [device_classes(table, f) for f in range(len(fleets))]
    code = check_gate_classes([c[1] for c in classes], max_groups, criterion)
    if not pos:
        return [[_NO_POINT] * R for _ in fleets]
    # the packer's error that depends on kappa's head, over the heads that can occur: every is_head device and
    # the first device of every class
    par, heads = [], []
    for f, (cls, counts, order) in enumerate(classes):
        a = int(table.dev_off[f])
        firsts = order[np.concatenate([[0], np.cumsum(counts)[:-1]])]
        hs = np.union1d(firsts, np.flatnonzero(table.flags[a:a + len(cls)] & DEV_HEAD))
        par += [f] * len(hs)
        heads += (a + hs).tolist()
    check_item_heads(fleets, table, np.asarray(par, np.int64), np.asarray(heads, np.int64), model)
    status, _, gcode, _, _ = solve_partition_classes_table(table, np.concatenate([c[0] for c in classes]), model, pos,
                                                           kv_factor, R, code, device)
    items, at = [], {}
    for f in range(len(fleets)):
        for r in range(1, R + 1):
            if int(status[f, r - 1]) == STATUS_OPTIMAL:
                at[(f, r)] = len(items)
                items += [(f, g) for g in _class_groups(gcode[f, r - 1, :r], classes[f][1], classes[f][2])]
    res = halda_solve_subfleets(fleets, model, items, k_candidates, kv_bits=kv_bits, device=device) if items else []
    out = []
    for f in range(len(fleets)):
        pts = []
        for r in range(1, R + 1):
            j = at.get((f, r))
            rs = None if j is None else res[j:j + r]
            if rs is None or any(x is None for x in rs):
                pts.append(_NO_POINT)
                continue
            pts.append(PartitionPoint([list(items[j + g][1]) for g in range(r)], list(rs),
                                      combine([x.obj_value for x in rs], criterion)))
        out.append(pts)
    return out


def halda_partition_frontier(
    devs: Sequence[DeviceProfile],
    model: ModelProfile,
    max_groups: int,
    criterion: str = "max",
    k_candidates: Optional[Iterable[int]] = None,
    kv_bits: str = "8bit",
    device: int = 0,
    route: str = "masks",
) -> List[PartitionPoint]:
    """The partition frontier of one fleet: point r (at index r - 1) is the best split of `devs` into exactly r
    groups, r = 1 .. max_groups; point 1 is the unsplit fleet. Each group's result equals
    `halda_solve_subfleets([devs], model, [(0, group)])[0]` bit for bit. The errors of
    halda_partition_frontier_batch."""
    return halda_partition_frontier_batch([list(devs)], model, max_groups, criterion, k_candidates, kv_bits, device,
                                          route)[0]


def halda_partition(
    devs: Sequence[DeviceProfile],
    model: ModelProfile,
    groups: int,
    criterion: str = "max",
    k_candidates: Optional[Iterable[int]] = None,
    kv_bits: str = "8bit",
    device: int = 0,
    route: str = "masks",
) -> PartitionPoint:
    """The best split of `devs` into exactly `groups` groups. RuntimeError when there is none."""
    pt = halda_partition_frontier(devs, model, groups, criterion, k_candidates, kv_bits, device, route)[-1]
    if pt.groups is None:
        raise RuntimeError(f"No feasible partition into {groups} groups.")
    return pt
