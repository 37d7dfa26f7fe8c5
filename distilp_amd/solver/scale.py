"""Scale-in and scale-out of a live fleet: WHICH devices to drop (or, from a pool, to add) under a budget of
released layers (libhalda `halda_solve_change_subsets`).

`halda_subset_frontier` picks devices but re-solves from scratch; `halda_failover_frontiers` honours the running
plan but only for the lists the caller spells out. Here the candidates are `subsets.py`'s -- the fleet without d
of its droppable devices (all but `keep`), enumerated by d ascending and, within one d, by their ascending
dropped-index lists in lexicographic order -- and a candidate's value at point p is `change.py`'s: the best plan of
its list that takes at most p layers off the kept devices, which hold the incumbent's layers. The GPU forms every
candidate from one 64-bit combo, runs the change kernel on them d by d and keeps, per (fleet, d, p), the arg-min
on the device (the earliest candidate among equal objectives): only the grid crosses PCIe.

The device orders candidates by the objective it forms. Each cell's ChangePoint is then built by a follow-up
`halda_change_frontiers` call over the distinct winning lists (one per d and k), so a cell's `point` is
`halda_failover_frontiers(devs, model, incumbent, max_released, lost=[dropped])[0][p]` field for field, bit for bit;
and along p the strict running minimum is taken again on these host-formed obj_values, as change.py does for its
own frontier: where the previous cell's list is strictly better at p than the device's pick, the cell keeps that
list (its point p, which the budget also admits).

Scale-out is the same call on `devs + pool`: every device of `devs` is kept, the pool holds nothing (w0 = 0), and
"add a of the q pool devices" is d = q - a. The tie order is therefore the DROPPED-list order: among equal
objectives the candidate whose left-out pool indices come first wins, so for a = 1 a tie goes to the LAST pool device.
"""

from __future__ import annotations

import ctypes
import math
import numbers
from dataclasses import dataclass
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._abi import HaldaChangeSubsetFrontierC, HaldaChangeSubsetsC
from ._libhalda import STATUS_OPTIMAL, get_context, ptr
from .bounds import INT32_MAX
from .budget import check_incumbent
from .change import ChangePoint, check_gate, check_released, halda_change_frontiers
from .coefficients import HALDAResult
from .fleets import _host_struct, fleet_table, model_struct
from .fleets import _bind as _bind_scale  # noqa: F401 -- the identity, for callers from before load_library bound all
from .lower import kv_bits_to_factor
from .plans import Incumbent
from .subsets import MAX_DEVICES, SUBSETS_MAX, candidate_lists, droppable

CHUNK_BYTES = 256 << 20  # csrc/halda.hip kChangeSubsetsChunkBytes: the scratch cap of one launch
FIXED_BYTES = 4096       # kChangeSubsetsFixedBytes
MAX_DROP = 63

SolveLists = Callable[[int, List[List[int]]], List[List[ChangePoint]]]


def set_change_subsets_chunk(ctx, nbytes: int) -> None:
    """halda_set_change_subsets_chunk on a HaldaContext: the scratch cap of one launch (0: the default)."""
    ctx.call("halda_set_change_subsets_chunk", ctx.ctx, int(nbytes), lock=False)


# ---------------------------------------------------------------- the gate's arithmetic
def launch_bytes(length: int, max_p: int, n_items: int) -> int:
    """halda_change_subsets_launch_bytes: the scratch of one launch of n_items candidates of `length` listed
    devices -- parent, sub_off and the four per-point arrays per candidate; sub_idx, w0 / w_min / w_max and the
    two planes per listed device; 4096 fixed."""
    P1 = int(max_p) + 1
    return FIXED_BYTES + int(n_items) * (12 + 20 * P1 + int(length) * (16 + 8 * P1))


def max_deficit(w0: Sequence[int], slots: Sequence[int], d: int, W: int) -> int:
    """halda_change_subsets_max_deficit: the largest deficit of the candidates with d of `slots` dropped --
    W - sum w0 plus the d largest droppable w0."""
    can = sorted((int(w0[i]) for i in slots), reverse=True)
    if d < 0 or d > len(can):
        raise ValueError(f"d = {d} is outside 0 .. {len(can)} droppable devices")
    return int(W) - sum(int(v) for v in w0) + sum(can[:d])


def scale_count(q: int, M: int, min_drop: int, max_drop: int) -> int:
    """The candidates of a fleet of M devices, q droppable, over d = min_drop .. min(max_drop, q, M - 1)."""
    return sum(math.comb(q, d) for d in range(min_drop, min(max_drop, q, M - 1) + 1))


def check_drops(min_drop, max_drop) -> Tuple[int, int]:
    """(min_drop, max_drop) as ints with 0 <= min_drop <= max_drop <= 63; ValueError otherwise."""
    for name, v in (("min_drop", min_drop), ("max_drop", max_drop)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f"{name}: {v!r} is not an integer")
    if min_drop < 0:
        raise ValueError("min_drop must be >= 0")
    if max_drop < min_drop:
        raise ValueError(f"max_drop = {max_drop} is below min_drop = {min_drop}")
    if max_drop > MAX_DROP:
        raise ValueError(f"max_drop = {max_drop} exceeds {MAX_DROP}")
    return int(min_drop), int(max_drop)


def check_scale_gate(sizes: Sequence[int], slots: Sequence[Sequence[int]], w0s: Sequence[Sequence[int]], W: int, k: int,
                     min_drop: int, max_drop: int, max_p: int) -> List[Optional[int]]:
    """The call's gate, from the shapes and w0 alone (what halda_solve_change_subsets refuses with HALDA_E_ARG):
    ValueError outside it. Returns, per d of the range, that d's largest deficit (None: no fleet admits d)."""
    tops: List[Optional[int]] = [None] * (max_drop - min_drop + 1)
    lens = [[0, MAX_DEVICES] for _ in tops]
    any_d = False
    for f, (M, sl, w0) in enumerate(zip(sizes, slots, w0s)):
        if M < 1 or M > MAX_DEVICES:
            raise ValueError(f"scale-in needs fleets of 1 .. {MAX_DEVICES} devices, fleet {f} has {M}")
        if len(w0) != M:
            raise ValueError(f"fleet {f}: w0 of {len(w0)} entries for {M} devices")
        if any(int(v) < 0 for v in w0):
            raise ValueError(f"fleet {f}: w0: every entry must be >= 0")
        if sum(int(v) for v in w0) > W:
            raise ValueError(f"fleet {f}: w0 sums to {sum(int(v) for v in w0)}, above L // k = {W}")
        lim = min(len(sl), M - 1)
        n = scale_count(len(sl), M, min_drop, max_drop)
        if n > SUBSETS_MAX:
            raise ValueError(f"{n} candidate sub-fleets ({len(sl)} droppable devices, {min_drop} .. "
                             f"{min(max_drop, lim)} dropped) exceed the limit of {SUBSETS_MAX}: lower max_drop or keep "
                             f"more devices")
        for d in range(min_drop, min(max_drop, lim) + 1):
            any_d = True
            D = max_deficit(w0, sl, d, W)
            j = d - min_drop
            tops[j] = D if tops[j] is None else max(tops[j], D)
            lens[j] = [max(lens[j][0], M - d), min(lens[j][1], M - d)]
    if not any_d:
        raise ValueError(f"min_drop = {min_drop} is beyond min(droppable devices, M - 1) of every fleet")
    for j, top in enumerate(tops):
        if top is not None:
            check_gate(lens[j][0], lens[j][1], max_p, top, k)
    return tops


# ---------------------------------------------------------------- the C call
@dataclass
class ScaleSolve:
    """halda_solve_change_subsets' grid: status / obj / dropped_mask / loaded / released [n_fleets, D1, P + 1] and
    w / n [n_fleets, D1, P + 1, 64] by PARENT device. obj is the GPU-formed objective."""

    status: np.ndarray
    obj: np.ndarray
    dropped_mask: np.ndarray
    loaded: np.ndarray
    released: np.ndarray
    w: np.ndarray
    n: np.ndarray
    k: int
    min_drop: int
    max_drop: int
    max_p: int


def solve_change_subsets_table(table, model: ModelProfile, k: int, w0: np.ndarray, min_drop: int, max_drop: int,
                               max_p: int, kv_factor: float, keep_masks: Optional[np.ndarray] = None,
                               w_min: Optional[np.ndarray] = None, w_max: Optional[np.ndarray] = None,
                               device: int = 0) -> ScaleSolve:
    """One halda_solve_change_subsets_host call on a packed table; w0 / w_min / w_max are int32 arrays per device
    of the table (laid out by dev_off), keep_masks uint64 per fleet or None. RuntimeError (HALDA_E_ARG) for a
    call outside the gate."""
    ctx = get_context(device)
    nf, D1, P1 = table.n_fleets, int(max_drop) - int(min_drop) + 1, int(max_p) + 1
    if D1 < 1 or P1 < 1:
        raise ValueError("needs min_drop <= max_drop and max_p >= 0")
    out = ScaleSolve(status=np.zeros((nf, D1, P1), np.int32), obj=np.zeros((nf, D1, P1)),
                     dropped_mask=np.zeros((nf, D1, P1), np.uint64), loaded=np.zeros((nf, D1, P1), np.int32),
                     released=np.zeros((nf, D1, P1), np.int32), w=np.zeros((nf, D1, P1, 64), np.int32),
                     n=np.zeros((nf, D1, P1, 64), np.int32), k=int(k), min_drop=int(min_drop), max_drop=int(max_drop),
                     max_p=int(max_p))
    fs, hold = _host_struct(table)
    nd = int(table.dev_off[nf])
    arrs = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (w0, w_min, w_max)]
    for a in arrs:
        if a is not None and len(a) != nd:
            raise ValueError(f"an array of {len(a)} entries for a table of {nd} devices")
    km = None if keep_masks is None else np.ascontiguousarray(keep_masks, np.uint64)
    sub = HaldaChangeSubsetsC(ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), int(min_drop), int(max_drop), int(max_p), ptr(km))
    fr = HaldaChangeSubsetFrontierC(*(ptr(getattr(out, f)) for f in
                                      ("status", "obj", "dropped_mask", "loaded", "released", "w", "n")))
    m = model_struct(model, kv_factor)
    ctx.call("halda_solve_change_subsets_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), int(k), ctypes.byref(sub),
             ctypes.byref(fr))
    del hold
    return out


# ---------------------------------------------------------------- the Python entries
@dataclass(frozen=True)
class ScalePoint:
    """Cell (d, p) of a scale-in frontier: the best candidate with exactly d devices dropped at a budget of p
    released layers -- the dropped and kept device indices (ascending, into the fleet; for scale-out into
    devs + pool) and the ChangePoint of the kept list (plan indexed within it). `added` (scale-out only): the
    pool indices that joined. Without a plan: dropped = kept = [] and change.py's empty point."""

    dropped: List[int]
    kept: List[int]
    point: ChangePoint
    added: Optional[List[int]] = None


def _empty(p: int, added=None) -> ScalePoint:
    return ScalePoint([], [], ChangePoint(p, None, math.inf, 0, 0, math.inf), added)


def _row(P: int, picks: List[Optional[Tuple[int, ...]]], frontier_of) -> List[ScalePoint]:
    """One row (one d) from the per-p picks (kept tuples, None: no plan) and `frontier_of(kept)`, the kept list's
    host-formed frontier: the strict running minimum over p -- where the previous cell's list is strictly better at
    p than the pick (or there is no pick), the cell keeps that list."""
    row, prev = [], None
    for p in range(P + 1):
        cur = picks[p]
        if cur is not None and frontier_of(cur)[p].plan is None:
            cur = None
        if prev is not None and frontier_of(prev)[p].plan is not None and (
                cur is None or frontier_of(prev)[p].obj_value < frontier_of(cur)[p].obj_value):
            cur = prev
        row.append(cur)
        prev = cur if cur is not None else prev
    return row


def _picks_by_lists(M: int, slots: Sequence[int], d: int, P: int, solve) -> Tuple[List[Optional[tuple]], dict]:
    """The picks of one (fleet, d) by enumeration: every candidate's frontier through `solve`, per p the strict
    earliest arg-min (the specification of the device's pick)."""
    # d <= M - 1, as on the device: the empty fleet is no candidate
    cands = [tuple(k) for _, k in candidate_lists(M, slots, d)] if d <= min(len(slots), M - 1) else []
    frs =solve([list(c) for c in cands]) if cands else []
    picks = []
    for p in range(P + 1):
        best, least = None, math.inf
        for c, fr in zip(cands, frs):
            if fr[p].plan is not None and (best is None or fr[p].obj_value < least):  # strict: the earliest stays
                best, least = c, fr[p].obj_value
        picks.append(best)
    return picks, dict(zip(cands, frs))


def _mask(idx: Iterable[int]) -> int:
    return sum(1 << int(i) for i in idx)


def _scale_core(fleets, model, ks, w0s, slots, min_drop, max_drop, P, kv_bits, los, his, device, solve_lists):
    """Per fleet [d - min_drop][p] of (dropped, kept, ChangePoint) or None. ks / w0s / slots / los / his per fleet
    (los / his: per-device bound lists or None)."""
    L = int(model.L)
    sizes = [len(d) for d in fleets]
    D1 = max_drop - min_drop + 1
    for k in sorted(set(ks)):
        grp = [f for f in range(len(fleets)) if ks[f] == k]
        check_scale_gate([sizes[f] for f in grp], [slots[f] for f in grp], [w0s[f] for f in grp], L // k, k, min_drop,
                         max_drop, P)
    out: List[Optional[list]] = [None] * len(fleets)
    if solve_lists is not None:
        for f in range(len(fleets)):
            rows = []
            for d in range(min_drop, max_drop + 1):
                picks, frs = _picks_by_lists(sizes[f], slots[f], d, P, lambda ls, f=f: solve_lists(f, ls))
                rows.append((_row(P, picks, frs.__getitem__), frs))
            out[f] = rows
        return out
    kv_factor = kv_bits_to_factor(kv_bits)
    for k in sorted(set(ks)):
        grp = [f for f in range(len(fleets)) if ks[f] == k]
        sub = [fleets[f] for f in grp]
        table = fleet_table(sub, model)
        w0 = np.concatenate([np.asarray(w0s[f], np.int32) for f in grp])
        bound = lambda bs, fill: None if all(bs[f] is None for f in grp) else np.concatenate(  # noqa: E731
            [np.full(sizes[f], fill, np.int32) if bs[f] is None else
             np.clip(np.asarray(bs[f], np.int64), -INT32_MAX, INT32_MAX).astype(np.int32) for f in grp])
        masks = np.asarray([_mask(i for i in range(sizes[f]) if i not in set(slots[f])) for f in grp], np.uint64)
        res = solve_change_subsets_table(table, model, k, w0, min_drop, max_drop, P, kv_factor, masks, bound(los, 0),
                                         bound(his, INT32_MAX), device)
        rows = {f: [] for f in grp}
        for j in range(D1):
            # the distinct winning lists of this d, one follow-up call
            picks, items, at = {}, [], {}
            for g, f in enumerate(grp):
                pk = []
                for p in range(P + 1):
                    if int(res.status[g, j, p]) != STATUS_OPTIMAL:
                        pk.append(None)
                        continue
                    m = int(res.dropped_mask[g, j, p])
                    kept = tuple(i for i in range(sizes[f]) if not (m >> i) & 1)
                    pk.append(kept)
                    if (g, kept) not in at:
                        at[(g, kept)] = len(items)
                        items.append((g, kept))
                picks[f] = pk
            frs = halda_change_frontiers(
                sub, model, [(g, list(s)) for g, s in items], k, [[w0s[grp[g]][i] for i in s] for g, s in items], P,
                kv_bits, None if all(los[f] is None for f in grp) else
                [None if los[grp[g]] is None else [los[grp[g]][i] for i in s] for g, s in items],
                None if all(his[f] is None for f in grp) else
                [None if his[grp[g]] is None else [his[grp[g]][i] for i in s] for g, s in items], device) if items else []
            for g, f in enumerate(grp):
                of = {s: frs[i] for (gg, s), i in at.items() if gg == g}
                rows[f].append((_row(P, picks[f], of.__getitem__), of))
        for f in grp:
            out[f] = rows[f]
    return out


def _points(M: int, rows, added_of=None) -> List[List[ScalePoint]]:
    out = []
    for row, frs in rows:
        pts = []
        for p, kept in enumerate(row):
            if kept is None:
                pts.append(_empty(p, None if added_of is None else []))
                continue
            gone = [i for i in range(M) if i not in set(kept)]
            pts.append(ScalePoint(gone, list(kept), frs[kept][p], None if added_of is None else added_of(kept)))
        out.append(pts)
    return out


def _check_bound_lists(fleets, w_min, w_max):
    out = []
    for name, b in (("w_min", w_min), ("w_max", w_max)):
        if b is None:
            out.append([None] * len(fleets))
            continue
        if len(b) != len(fleets):
            raise ValueError(f"{len(b)} {name} entries for {len(fleets)} fleets")
        for f, a in enumerate(b):
            if a is not None and len(a) != len(fleets[f]):
                raise ValueError(f"{name}: {len(a)} entries for a fleet of {len(fleets[f])} devices")
        out.append([None if a is None else [int(v) for v in a] for a in b])
    return out


def halda_scale_in_frontier_batch(fleets: Sequence[Sequence[DeviceProfile]], model: ModelProfile,
                                  incumbents: Sequence[Incumbent], max_drop: int, max_released: int,
                                  keep: Optional[Sequence[Optional[Iterable[int]]]] = None, min_drop: int = 0,
                                  kv_bits: str = "8bit", w_min: Optional[Sequence[Optional[Sequence[int]]]] = None,
                                  w_max: Optional[Sequence[Optional[Sequence[int]]]] = None, device: int = 0,
                                  _solve_lists: Optional[SolveLists] = None) -> List[List[List[ScalePoint]]]:
    """Per fleet its scale-in frontier [d - min_drop][p], d = min_drop .. max_drop, p = 0 .. max_released: the best
    way to hand back exactly d of the droppable devices (all but `keep[f]`) while taking at most p layers off the
    others, which hold `incumbents[f]`'s layers. One packed table and one C call per distinct incumbent k (fleets of
    mixed sizes allowed; a fleet that cannot drop d devices has an empty row there), then one halda_change_frontiers
    call per (k, d) over the distinct winning lists. w_min / w_max: per fleet a list per device, or None.
    ValueError / IndexError before any GPU work for a bad incumbent, budget, keep index, d range, more than 2^20
    candidates in a fleet, more than 64 devices, or a d whose list length and largest deficit fall outside the
    change kernel's gate. `_solve_lists(f, lists)` (tests): the change frontiers (max_released + 1 ChangePoints
    each) of index lists of fleet f, in place of the GPU."""
    fleets = [list(d) for d in fleets]
    P = check_released(max_released)
    min_drop, max_drop = check_drops(min_drop, max_drop)
    if len(incumbents) != len(fleets):
        raise ValueError(f"{len(incumbents)} incumbents for {len(fleets)} fleets")
    if keep is not None and len(keep) != len(fleets):
        raise ValueError(f"{len(keep)} keep entries for {len(fleets)} fleets")
    los, his = _check_bound_lists(fleets, w_min, w_max)
    ks, w0s, slots = [], [], []
    for f, devs in enumerate(fleets):
        if not devs:
            raise IndexError("list index out of range")  # the reference's kappa on an empty fleet
        if len(devs) > MAX_DEVICES:
            raise ValueError(f"scale-in needs fleets of at most {MAX_DEVICES} devices, fleet {f} has {len(devs)}")
        k, w, _ = check_incumbent(incumbents[f], len(devs), int(model.L))
        ks.append(k)
        w0s.append(w)
        slots.append(droppable(len(devs), None if keep is None else keep[f]))
    if not fleets:
        return []
    rows = _scale_core(fleets, model, ks, w0s, slots, min_drop, max_drop, P, kv_bits, los, his, device, _solve_lists)
    return [_points(len(fleets[f]), rows[f]) for f in range(len(fleets))]


def halda_scale_in_frontier(devs: Sequence[DeviceProfile], model: ModelProfile, incumbent: Incumbent, max_drop: int,
                            max_released: int, keep: Optional[Iterable[int]] = None, min_drop: int = 0,
                            kv_bits: str = "8bit", w_min: Optional[Sequence[int]] = None,
                            w_max: Optional[Sequence[int]] = None, device: int = 0,
                            _solve_lists: Optional[Callable[[List[List[int]]], List[List[ChangePoint]]]] = None
                            ) -> List[List[ScalePoint]]:
    """The scale-in frontier of one fleet, [d - min_drop][p] of ScalePoint: cell (d, p) names the d devices to
    hand back and the plan to move to when at most p layers may be taken off the others. Its `point` equals
    `halda_failover_frontiers(devs, model, incumbent, max_released, lost=[dropped])[0][p]` bit for bit; row 0 is
    `halda_change_frontier` of the whole fleet. Errors as halda_scale_in_frontier_batch."""
    hook = None if _solve_lists is None else (lambda f, ls: _solve_lists(ls))
    return halda_scale_in_frontier_batch([list(devs)], model, [incumbent], max_drop, max_released,
                                         None if keep is None else [keep], min_drop, kv_bits,
                                         None if w_min is None else [w_min], None if w_max is None else [w_max], device,
                                         hook)[0]


def halda_scale_in(devs: Sequence[DeviceProfile], model: ModelProfile, incumbent: Incumbent, drop: int,
                   max_released: int, keep: Optional[Iterable[int]] = None, kv_bits: str = "8bit", device: int = 0,
                   _solve_lists=None) -> Tuple[List[int], HALDAResult]:
    """Which `drop` devices to hand back, and the plan to move to (indexed within the kept devices), when at most
    max_released layers may be taken off the others: the last point of row `drop`. RuntimeError when there is
    none."""
    pt = halda_scale_in_frontier(devs, model, incumbent, drop, max_released, keep, drop, kv_bits, device=device,
                                 _solve_lists=_solve_lists)[0][-1]
    if pt.point.plan is None:
        raise RuntimeError("No feasible MILP found within the released-layer budget for any choice of devices.")
    return list(pt.dropped), pt.point.plan


def halda_scale_out_frontier(devs: Sequence[DeviceProfile], pool: Sequence[DeviceProfile], model: ModelProfile,
                             incumbent: Incumbent, max_add: int, max_released: int, kv_bits: str = "8bit",
                             device: int = 0, _solve_lists=None) -> List[List[ScalePoint]]:
    """The scale-out frontier [a][p], a = 0 .. max_add: the best a devices of `pool` to add to the running fleet when
    at most p layers may be taken off its devices; `added` holds their pool indices, `kept` / `dropped` index
    devs + pool, and the plan is indexed within `kept`. A joiner holds nothing and must receive a layer, so with a
    full incumbent point 0 of every row a >= 1 has no plan. Row 1 is the per-p best of `halda_join_frontiers`.
    Ties: the candidate order is that of the LEFT-OUT pool indices (ascending lists, lexicographic), so among equal
    objectives the later pool devices are added. ValueError for max_add outside 0 .. len(pool)."""
    devs, pool = list(devs), list(pool)
    M, q = len(devs), len(pool)
    P = check_released(max_released)
    if isinstance(max_add, bool) or not isinstance(max_add, numbers.Integral) or not 0 <= max_add <= q:
        raise ValueError(f"max_add = {max_add!r} must be an integer in 0 .. {q} (the pool)")
    if not devs:
        raise IndexError("list index out of range")
    if M + q > MAX_DEVICES:
        raise ValueError(f"scale-out needs at most {MAX_DEVICES} devices in fleet and pool, got {M + q}")
    k, w, _ = check_incumbent(incumbent, M, int(model.L))
    min_drop, max_drop = check_drops(q - int(max_add), q)
    hook = None if _solve_lists is None else (lambda f, ls: _solve_lists(ls))
    rows = _scale_core([devs + pool], model, [k], [list(w) + [0] * q], [list(range(M, M + q))], min_drop, max_drop, P,
                       kv_bits, [None], [None], device, hook)[0]
    pts = _points(M + q, rows, lambda kept: [i - M for i in kept if i >= M])
    return pts[::-1]  # row a is d = q - a
