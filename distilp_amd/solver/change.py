"""Re-placement of a live fleet after a device is lost or joins (libhalda `halda_solve_change`): the exact
frontier "how good a plan can I reach if I disturb the surviving devices by at most p layers".

`halda_move_frontier` answers that on an unchanged fleet only (sum w0 = W, every w0_i >= 1), and
`halda_leave_one_out` / `halda_solve_subfleets` re-solve a changed fleet from scratch and may reshuffle every
survivor. Here an item is a sub-fleet of a packed parent fleet (halda_solve_subfleets' items) with the layers
each listed device holds NOW: w0_i >= 0, 0 for a device that just joined. The deficit D = W - sum w0 >= 0 is
what the lost devices held (W = L // k at the incumbent's k). Writing delta_i = w_i - w0_i,

    loaded   = sum max(0,  delta_i)   layers some device must newly load,
    released = sum max(0, -delta_i)   layers taken off a surviving device,      loaded = D + released.

Point p of the frontier (p = 0 .. max_released) is the optimum of the list's fixed-k problem over the plans with
released <= p; n, the slacks, z and C are re-optimised. Point 0 deals the orphans out and disturbs no survivor;
with D = 0 and a joiner it has no plan (every listed device needs w >= 1). One GPU call answers every point of
every item -- an N-1 contingency table is one call on one packed parent.
"""

from __future__ import annotations

import ctypes
import math
import numbers
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._abi import HaldaChangeC, HaldaChangeFrontierC, HaldaSubfleetsC
from ._libhalda import STATUS_OPTIMAL, get_context, ptr
from .bounds import INT32_MAX, check_bounds
from .budget import check_incumbent, distinct_plans, frontier_lds_bytes, host_frontier
from .coefficients import HALDAResult, assign_sets
from .fleets import FleetTable, _host_struct, fleet_table, model_struct
from .fleets import _bind as _bind_change  # noqa: F401 -- the identity, for callers from before load_library bound all
from .lower import kv_bits_to_factor
from .plans import Incumbent, halda_evaluate_plans_batch
from .subfleets import halda_solve_subfleets, pack_items

LDS_BUDGET = 160 * 1024  # csrc/halda.hip kLdsBudget
MAX_P = 63               # one lane per frontier point
MAX_DEVICES = 64         # one lane per listed device
MAX_ENTRY = 254          # 2 P + max_deficit: a table index is one byte, 255 marks an unreached state

Lost = Union[int, Sequence[int]]


def change_lds_bytes(max_devices: int, max_p: int, max_deficit: int, k: int) -> int:
    """halda_sweep_change_kernel's slice (change_slice, the figure halda_change_lds_bytes returns): rows of
    RS = (2 P + Dmax + 1) | 1 entries and S = (P + 1)(Dmax + P + 1) states."""
    P, D = int(max_p), int(max_deficit)
    return frontier_lds_bytes(max_devices, P, (2 * P + D + 1) | 1, (P + 1) * (D + P + 1), k)


def check_gate(max_devices: int, min_devices: int, max_p: int, max_deficit: int, k: int) -> None:
    """The launch's gate, from the shapes alone: ValueError outside it (there is no other route)."""
    if min_devices < 1 or max_devices > MAX_DEVICES:
        raise ValueError(f"a change frontier needs lists of 1 .. {MAX_DEVICES} devices, got {min_devices} .. "
                         f"{max_devices}")
    if max_p < 0 or max_p > MAX_P:
        raise ValueError(f"max_released = {max_p} exceeds {MAX_P}" if max_p > MAX_P else "max_released must be >= 0")
    if max_deficit < 0:
        raise ValueError("max_deficit must be >= 0")
    if 2 * max_p + max_deficit > MAX_ENTRY:
        raise ValueError(f"2 * max_released + deficit = {2 * max_p + max_deficit} exceeds {MAX_ENTRY}")
    need = change_lds_bytes(max_devices, max_p, max_deficit, k)
    if need > LDS_BUDGET:
        raise ValueError(f"{max_p} released layers with a deficit of {max_deficit} on lists of up to {max_devices} "
                         f"devices need {need} B of LDS per item, beyond the {LDS_BUDGET} B budget: lower max_released")


def check_released(max_released) -> int:
    """P of a budget of released layers. ValueError for a negative or non-integer value."""
    if isinstance(max_released, bool) or not isinstance(max_released, numbers.Integral):
        raise ValueError(f"max_released: {max_released!r} is not an integer")
    if max_released < 0:
        raise ValueError("max_released must be >= 0")
    return int(max_released)


def check_w0(sub_off: np.ndarray, w0: np.ndarray, W: int, max_deficit: Optional[int] = None) -> int:
    """The largest deficit D = W - sum w0 over the items of w0 (laid out by sub_off). ValueError for a wrong
    length, some w0_i < 0, an item with D < 0 or with D > max_deficit (what halda_solve_change_host rejects)."""
    w0 = np.asarray(w0, np.int64).reshape(-1)
    if len(w0) != int(sub_off[-1]):
        raise ValueError(f"w0 of {len(w0)} entries for {int(sub_off[-1])} listed devices")
    if len(w0) and int(w0.min()) < 0:
        raise ValueError("w0: every entry must be >= 0")
    D = int(W) - np.add.reduceat(w0, sub_off[:-1]) if len(sub_off) > 1 else np.zeros(0, np.int64)
    bad = np.flatnonzero(D < 0)
    if len(bad):
        i = int(bad[0])
        raise ValueError(f"item {i}: w0 sums to {int(W) - int(D[i])}, above L // k = {int(W)} (a negative deficit)")
    top = int(D.max()) if len(D) else 0
    if max_deficit is not None and top > max_deficit:
        raise ValueError(f"a deficit of {top} layers exceeds max_deficit = {max_deficit}")
    return top


@dataclass(frozen=True)
class ChangePoint:
    """Point p of a change frontier: released_budget = p, the best plan that takes at most p layers off the
    listed devices (None where there is none; w / n indexed within the list), its obj_value (inf without a
    plan), the layers it really loads and releases (loaded = deficit + released, released <= p), and
    regret = obj_value minus the list's free optimum at the same k (>= 0 up to rounding; inf without a plan)."""

    released_budget: int
    plan: Optional[HALDAResult]
    obj_value: float
    loaded: int
    released: int
    regret: float


@dataclass
class ChangeSolve:
    """halda_solve_change's arrays: status / obj / loaded / released [n_items, P + 1], w / n [P + 1, sub_off[-1]].
    obj is the GPU-formed objective (halda_eval_plans' bits for the same plan on the materialised list)."""

    status: np.ndarray
    obj: np.ndarray
    loaded: np.ndarray
    released: np.ndarray
    w: np.ndarray
    n: np.ndarray
    k: int
    max_p: int
    max_deficit: int


def solve_change_table(table: FleetTable, model: ModelProfile, k: int, items, w0: np.ndarray, max_p: int,
                       kv_factor: float, w_min: Optional[np.ndarray] = None, w_max: Optional[np.ndarray] = None,
                       max_deficit: Optional[int] = None, device: int = 0) -> ChangeSolve:
    """One halda_solve_change_host call on a packed parent table. `items` is (parent, sub_off, sub_idx) as
    subfleets.pack_items returns them; w0 / w_min / w_max are int32 arrays laid out by sub_off. max_deficit
    None: the items' largest deficit. ValueError before any GPU work for a bad w0 or a shape outside the gate."""
    parent, sub_off, sub_idx = items
    lens = np.diff(sub_off)
    if int(k) < 1:
        raise ValueError(f"k = {k} must be positive")
    top = check_w0(sub_off, w0, int(model.L) // int(k), max_deficit)
    dmax = top if max_deficit is None else int(max_deficit)
    check_gate(int(lens.max()), int(lens.min()), int(max_p), dmax, int(k))
    ctx = get_context(device)
    n, tot, P1 = len(parent), int(sub_off[-1]), int(max_p) + 1
    out = ChangeSolve(status=np.zeros((n, P1), np.int32), obj=np.zeros((n, P1)), loaded=np.zeros((n, P1), np.int32),
                      released=np.zeros((n, P1), np.int32), w=np.zeros((P1, tot), np.int32),
                      n=np.zeros((P1, tot), np.int32), k=int(k), max_p=int(max_p), max_deficit=dmax)
    fs, keep = _host_struct(table)
    arrs = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (w0, w_min, w_max)]
    for a in arrs[1:]:
        if a is not None and len(a) != tot:
            raise ValueError(f"bound array of {len(a)} entries for {tot} listed devices")
    parent, sub_idx = np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(sub_idx, np.int32)
    sub_off = np.ascontiguousarray(sub_off, np.int64)
    it = HaldaSubfleetsC(n, int(lens.min()), int(lens.max()), ptr(parent), ptr(sub_off), ptr(sub_idx))
    ch = HaldaChangeC(ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), int(max_p), dmax)
    fr = HaldaChangeFrontierC(tot, *(ptr(getattr(out, f)) for f in ("status", "obj", "loaded", "released", "w", "n")))
    m = model_struct(model, kv_factor)
    ctx.call("halda_solve_change_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it), int(k),
             ctypes.byref(ch), ctypes.byref(fr))
    del keep
    return out


def _flat_lists(lists, fill: int) -> Optional[np.ndarray]:
    """Per-item int lists (None: no bound) laid out by sub_off, None when no item has one."""
    if all(a is None for a in lists[0]):
        return None
    return np.concatenate([np.full(m, fill, np.int32) if a is None else
                           np.clip(np.asarray(a, np.int64), -INT32_MAX, INT32_MAX).astype(np.int32)
                           for a, m in zip(*lists)])


def halda_change_frontiers(fleets: Sequence[Sequence[DeviceProfile]], model: ModelProfile,
                           items: Sequence[Tuple[int, Sequence[int]]], k: int, w0s: Sequence[Sequence[int]],
                           max_released: int, kv_bits: str = "8bit",
                           w_min: Optional[Sequence[Optional[Sequence[int]]]] = None,
                           w_max: Optional[Sequence[Optional[Sequence[int]]]] = None,
                           device: int = 0) -> List[List[ChangePoint]]:
    """Per item (parent fleet, index list) the change frontier around w0s[i] (the layers its listed devices
    hold, in list order; zeros allowed): one ChangePoint per p = 0 .. max_released. ONE packed parent table and
    ONE kernel call for every item; one halda_solve_subfleets call gives the lists' free optima at k (for
    `regret`), and one evaluation call prices every distinct returned plan on its materialised list, so a
    point's obj_value is halda_evaluate_plan's of its plan bit for bit. w_min / w_max: per item a list of bounds
    in list order or None. ValueError / IndexError before any GPU work for malformed items, a bad w0 (a negative
    entry, a sum above L // k), a bad budget, or a shape outside the launch's gate."""
    kv_factor = kv_bits_to_factor(kv_bits)
    fleets = [list(d) for d in fleets]
    items = [(int(f), [int(j) for j in s]) for f, s in items]
    P = check_released(max_released)
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 1:
        raise ValueError(f"k = {k!r} must be a positive integer")
    k = int(k)
    if len(w0s) != len(items):
        raise ValueError(f"{len(w0s)} w0 lists for {len(items)} items")
    for name, b in (("w_min", w_min), ("w_max", w_max)):
        if b is not None and len(b) != len(items):
            raise ValueError(f"{len(b)} {name} entries for {len(items)} items")
    if not items:
        return []
    packed = pack_items(np.asarray([len(d) for d in fleets], np.int64), items)
    lens = np.diff(packed[1])
    los, his = [], []
    for i, (_, s) in enumerate(items):
        if len(w0s[i]) != len(s):
            raise ValueError(f"item {i}: w0 of {len(w0s[i])} entries for a list of {len(s)} devices")
        lo, hi = check_bounds(None if w_min is None else w_min[i], None if w_max is None else w_max[i], len(s))
        los.append(lo)
        his.append(hi)
    w0 = np.concatenate([np.asarray([int(v) for v in a], np.int64) for a in w0s])
    if len(w0) and (int(w0.max()) > INT32_MAX or int(w0.min()) < -INT32_MAX):
        raise ValueError("w0: an entry does not fit 32 bits")
    top = check_w0(packed[1], w0, int(model.L) // k)
    check_gate(int(lens.max()), int(lens.min()), P, top, k)
    table = fleet_table(fleets, model)
    res = solve_change_table(table, model, k, packed, w0.astype(np.int32), P, kv_factor,
                             _flat_lists((los, lens), 0), _flat_lists((his, lens), INT32_MAX), top, device)
    raw = []  # per item [(w, n, loaded, released) or None per point]
    for i in range(len(items)):
        a, b = int(packed[1][i]), int(packed[1][i + 1])
        raw.append([([int(v) for v in res.w[p, a:b]], [int(v) for v in res.n[p, a:b]], int(res.loaded[i, p]),
                     int(res.released[i, p])) if int(res.status[i, p]) == STATUS_OPTIMAL else None
                    for p in range(P + 1)])
    free = halda_solve_subfleets(fleets, model, items, [k], kv_bits=kv_bits, device=device)
    # obj_value formed on the host as every entry of this package forms it: every distinct returned plan priced
    # on its materialised list in ONE evaluation call
    lists = [[fleets[f][j] for j in s] for f, s in items]
    need = distinct_plans(raw)
    ev = halda_evaluate_plans_batch([lists[i] for i, _ in need], model, [(k, *raw[i][p][:2]) for i, p in need],
                                    kv_bits, device) if need else []
    out = []
    for i, row in enumerate(host_frontier(raw, need, [e.obj_value for e in ev])):
        sets, pts = assign_sets(lists[i]), []
        base = free[i].obj_value if free[i] is not None else math.inf
        for p, c in enumerate(row):
            if c is None:
                pts.append(ChangePoint(p, None, math.inf, 0, 0, math.inf))
                continue
            (w, n, loaded, released), obj = c
            plan = HALDAResult(w=w, n=n, k=k, obj_value=obj, sets=sets)
            pts.append(ChangePoint(p, plan, obj, loaded, released, obj - base))
        out.append(pts)
    return out


def halda_change_frontier(devs: Sequence[DeviceProfile], model: ModelProfile, k: int, w0: Sequence[int],
                          max_released: int, kv_bits: str = "8bit", w_min: Optional[Sequence[int]] = None,
                          w_max: Optional[Sequence[int]] = None, device: int = 0) -> List[ChangePoint]:
    """The change frontier of one fleet AFTER the change: `devs` are the devices there are now, w0 the layers
    each holds (0 for a device that just joined; sum w0 <= L // k, the rest being orphaned layers)."""
    devs = list(devs)
    return halda_change_frontiers([devs], model, [(0, list(range(len(devs))))], k, [list(w0)], max_released, kv_bits,
                                  None if w_min is None else [w_min], None if w_max is None else [w_max], device)[0]


def _lost_lists(M: int, lost) -> List[List[int]]:
    """The entries of `lost` as sorted index lists; None: every single device (none for a one-device fleet)."""
    if lost is None:
        return [[i] for i in range(M)] if M > 1 else []
    out = []
    for e in lost:
        idx = [e] if isinstance(e, numbers.Integral) and not isinstance(e, bool) else list(e)
        for j in idx:
            if isinstance(j, bool) or not isinstance(j, numbers.Integral):
                raise ValueError(f"lost: {j!r} is not a device index")
            if j < 0 or j >= M:
                raise IndexError(f"lost: device index {j} out of range for a fleet of {M} devices")
        idx = sorted({int(j) for j in idx})
        if not idx:
            raise ValueError("lost: an entry names no device")
        if len(idx) == M:
            raise ValueError("lost: an entry leaves no device")
        out.append(idx)
    return out


def _sub(a: Optional[Sequence[int]], keep: Sequence[int]):
    return None if a is None else [a[j] for j in keep]


def halda_failover_frontiers(devs: Sequence[DeviceProfile], model: ModelProfile, incumbent: Incumbent,
                             max_released: int, lost: Optional[Sequence[Lost]] = None, kv_bits: str = "8bit",
                             w_min: Optional[Sequence[int]] = None, w_max: Optional[Sequence[int]] = None,
                             device: int = 0) -> List[List[ChangePoint]]:
    """The N-1 contingency table of a running plan: one change frontier per entry of `lost` (a device index or
    a tuple of them; default: every single device), for the fleet without those devices, the survivors holding
    the incumbent's layers. The fleet is packed ONCE and every entry is solved in ONE kernel call. Plans are
    indexed within the survivors' list (the fleet's order); w_min / w_max are per device of `devs`."""
    devs = list(devs)
    M = len(devs)
    P = check_released(max_released)
    k, w, _ = check_incumbent(incumbent, M, int(model.L))
    for name, b in (("w_min", w_min), ("w_max", w_max)):
        if b is not None and len(b) != M:
            raise ValueError(f"{name}: {len(b)} entries for a fleet of {M} devices")
    gone = _lost_lists(M, lost)
    keeps = [[j for j in range(M) if j not in set(g)] for g in gone]
    return halda_change_frontiers([devs], model, [(0, s) for s in keeps], k, [[w[j] for j in s] for s in keeps], P,
                                  kv_bits, None if w_min is None else [_sub(w_min, s) for s in keeps],
                                  None if w_max is None else [_sub(w_max, s) for s in keeps], device)


def halda_join_frontiers(devs: Sequence[DeviceProfile], pool: Sequence[DeviceProfile], model: ModelProfile,
                         incumbent: Incumbent, max_released: int, kv_bits: str = "8bit",
                         w_min: Optional[Sequence[int]] = None, w_max: Optional[Sequence[int]] = None,
                         device: int = 0) -> List[List[ChangePoint]]:
    """One change frontier per device of `pool` that joins the running fleet: the list is `devs` followed by
    that device, which holds nothing (w0 = 0) and must receive at least one layer, so point 0 has no plan. The
    parent is the fleet plus the pool, packed once; one kernel call. w_min / w_max are per device of `devs` (the
    joiner is unbounded)."""
    devs, pool = list(devs), list(pool)
    M = len(devs)
    P = check_released(max_released)
    k, w, _ = check_incumbent(incumbent, M, int(model.L))
    for name, b in (("w_min", w_min), ("w_max", w_max)):
        if b is not None and len(b) != M:
            raise ValueError(f"{name}: {len(b)} entries for a fleet of {M} devices")
    n = len(pool)
    return halda_change_frontiers([devs + pool], model, [(0, list(range(M)) + [M + j]) for j in range(n)], k,
                                  [list(w) + [0]] * n, P, kv_bits,
                                  None if w_min is None else [list(w_min) + [1]] * n,
                                  None if w_max is None else [list(w_max) + [INT32_MAX]] * n, device)


def halda_failover_plan(devs: Sequence[DeviceProfile], model: ModelProfile, incumbent: Incumbent, lost: Lost,
                        max_released: int, kv_bits: str = "8bit", device: int = 0) -> HALDAResult:
    """The plan to move to when `lost` (a device index or a tuple of them) drops out and at most max_released
    layers may be taken off the survivors: the frontier's last point. RuntimeError, as halda_solve raises it,
    when there is none."""
    r = halda_failover_frontiers(devs, model, incumbent, max_released, [lost], kv_bits, device=device)[0][-1].plan
    if r is None:
        raise RuntimeError("No feasible MILP found within the released-layer budget.")
    return r
