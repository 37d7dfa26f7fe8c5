"""A total move budget around a deployed plan (libhalda `halda_solve_fleets_budget`): the best plan within B
moved layers, and the whole frontier obj(B).

`halda_replace_within` re-optimises inside a per-device box: every device may move by D at once, and the one
large move a small total budget would allow is forbidden. The budget an operator usually holds is the other
one: how many layers may change device in total, sum_i |w_i - w0_i| <= B, because that is the amount of
weights that crosses the network. The constraint couples the devices, so it is no narrowing of column bounds;
the GPU solves it with a dynamic programme over "layers moved so far", which yields the optimum of every budget
0 .. B in the same pass -- the curve an operator picks the knee from.

Units: B is `moved_layers`' unit, sum |w_i - w0_i|. At the incumbent's k both plans sum to W = L // k, so the
sum is even: point p of the frontier (p = 0 .. B // 2) is the best plan that moves at most p layers onto other
devices (sum max(0, w_i - w0_i) <= p, hence moved_layers <= 2 p). n, the slacks, z and C are re-optimised
freely at every point; point 0 is "w pinned, n re-optimised".
"""

from __future__ import annotations

import ctypes
import math
import numbers
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._abi import HaldaBudgetC, HaldaFrontierC
from ._libhalda import STATUS_OPTIMAL, get_context, ptr
from .bounds import INT32_MAX, _int_list, check_bounds
from .coefficients import HALDAResult, assign_sets
from .fleets import FleetTable, _host_struct, fleet_table, model_struct
from .fleets import _bind as _bind_budget  # noqa: F401 -- the identity, for callers from before load_library bound all
from .lower import kv_bits_to_factor
from .plans import Incumbent, _as_plan, halda_evaluate_plans_batch

LDS_BUDGET = 160 * 1024  # csrc/halda.hip kLdsBudget
MAX_P = 63               # one lane per frontier point
MAX_DEVICES = 64         # one lane per device


def _align16(x: int) -> int:
    return (x + 15) & ~15


def frontier_lds_bytes(max_devices: int, max_p: int, RS: int, S: int, k: int) -> int:
    """The LDS slice of one wave of a frontier kernel (csrc/halda_sweep.hpp frontier_slice): the tables G and, for
    k > 1, H as max_devices rows of RS doubles, two value planes of S doubles, one arg-min byte plane of S per
    device, and the plans."""
    M, P = int(max_devices), int(max_p)
    o = _align16(M * RS * 8)
    o = _align16(o + (M * RS * 8 if k > 1 else 0))
    o = _align16(o + 2 * S * 8)
    o = _align16(o + M * S)
    o = _align16(o + M * 4)
    o = _align16(o + (P + 1) * M)
    o = _align16(o + (P + 1) * M * 4)
    return o


def budget_lds_bytes(max_devices: int, max_p: int, k: int) -> int:
    """halda_sweep_budget_kernel's slice (budget_slice, the figure halda_budget_lds_bytes returns): rows of
    2 P + 1 entries and S = (2 P + 1)(P + 1) states."""
    P = int(max_p)
    return frontier_lds_bytes(max_devices, P, 2 * P + 1, (2 * P + 1) * (P + 1), k)


def check_gate(max_devices: int, min_devices: int, max_p: int, k: int) -> None:
    """The launch's gate, from the shapes alone: ValueError outside it (there is no other route)."""
    if min_devices < 1 or max_devices > MAX_DEVICES:
        raise ValueError(f"a move frontier needs fleets of 1 .. {MAX_DEVICES} devices, got {min_devices} .. "
                         f"{max_devices}")
    if max_p > MAX_P:
        raise ValueError(f"max_moved_layers // 2 = {max_p} exceeds {MAX_P} (max_moved_layers <= {2 * MAX_P + 1})")
    need = budget_lds_bytes(max_devices, max_p, k)
    if need > LDS_BUDGET:
        raise ValueError(f"a budget of {max_p} moved layers on fleets of up to {max_devices} devices needs "
                         f"{need} B of LDS per fleet, beyond the {LDS_BUDGET} B budget: lower max_moved_layers")


def check_budget(max_moved_layers) -> int:
    """P = B // 2 of a budget B in moved_layers' unit. ValueError for a negative or non-integer B."""
    if isinstance(max_moved_layers, bool) or not isinstance(max_moved_layers, numbers.Integral):
        raise ValueError(f"max_moved_layers: {max_moved_layers!r} is not an integer")
    if max_moved_layers < 0:
        raise ValueError("max_moved_layers must be >= 0")
    return int(max_moved_layers) // 2


def check_incumbent(inc: Incumbent, M: int, L: int):
    """(k, w0, n0) of an incumbent. ValueError for None, a wrong length, k < 1, some w0_i < 1 or
    sum w0 != L // k."""
    p = _as_plan(inc)
    if p is None:
        raise ValueError("a move frontier needs an incumbent plan (a HALDAResult or (k, w, n)), got None")
    k, w0, n0 = p
    if isinstance(k, bool) or k < 1:
        raise ValueError(f"incumbent k = {k} must be positive")
    w0 = _int_list(w0, "incumbent w", M)
    n0 = _int_list(n0, "incumbent n", M)
    if any(v < 1 for v in w0):
        raise ValueError("incumbent w: every entry must be >= 1")
    if sum(w0) != L // k:
        raise ValueError(f"incumbent w sums to {sum(w0)}, not L // k = {L // k}")
    return int(k), w0, n0


@dataclass(frozen=True)
class FrontierPoint:
    """Point p of a move frontier: budget_layers = 2 p (moved_layers' unit), the best plan within it (None
    where there is none), its obj_value (inf without a plan), the layers it really moves,
    moved_layers = sum |w_i - w0_i| <= budget_layers, and regret = incumbent's obj_value on this fleet minus
    obj_value (inf for an infeasible incumbent, -inf where only the point has no plan)."""

    budget_layers: int
    plan: Optional[HALDAResult]
    obj_value: float
    moved_layers: int
    regret: float


@dataclass
class FrontierSolve:
    """halda_solve_fleets_budget's arrays: status / obj / moved [n_fleets, P + 1], w / n [P + 1, n_devices]. obj is
    the GPU-formed objective (halda_eval_plans' bits for the same plan); the entries below re-form it on the host."""

    status: np.ndarray
    obj: np.ndarray
    moved: np.ndarray
    w: np.ndarray
    n: np.ndarray
    k: int
    max_p: int


def distinct_plans(raw) -> List[tuple]:
    """The (row, point) pairs of a kernel frontier that need a price. raw[row][p] is a tuple (w, n, ...) or None
    (no plan); a point whose (w, n) is the previous point's shares its price."""
    return [(i, p) for i, pts in enumerate(raw) for p, r in enumerate(pts)
            if r is not None and (p == 0 or pts[p - 1] is None or pts[p - 1][:2] != r[:2])]


def host_frontier(raw, need, objs) -> List[list]:
    """Per row and point None (no plan) or (the point's tuple of raw, its obj_value), `objs` being the host-formed
    objectives of the plans at `need` = distinct_plans(raw). The kernel's prefix-min orders the points by the
    GPU-formed objective; two different plans within an ulp of each other can order the other way once re-formed
    on the host, so the running minimum is taken here too: such a point keeps the previous point's plan, which
    its budget also admits."""
    slot = dict(zip(need, objs))
    out = []
    for i, pts in enumerate(raw):
        row, obj = [], None
        for p, r in enumerate(pts):
            obj = slot.get((i, p), obj)
            if r is None:
                row.append(None)
            elif row and row[-1] is not None and row[-1][1] < obj:
                row.append(row[-1])
            else:
                row.append((r, obj))
        out.append(row)
    return out


def solve_budget_table(table: FleetTable, model: ModelProfile, k: int, w0: np.ndarray, max_p: int,
                       kv_factor: float, w_min: Optional[np.ndarray] = None, w_max: Optional[np.ndarray] = None,
                       device: int = 0) -> FrontierSolve:
    """One halda_solve_fleets_budget_host call on a packed table (w0 / w_min / w_max int32, device layout)."""
    sizes = table.sizes()
    check_gate(int(sizes.max()), int(sizes.min()), int(max_p), int(k))
    ctx = get_context(device)
    nf, nd, P1 = table.n_fleets, table.n_devices, int(max_p) + 1
    out = FrontierSolve(status=np.zeros((nf, P1), np.int32), obj=np.zeros((nf, P1)),
                        moved=np.zeros((nf, P1), np.int32), w=np.zeros((P1, nd), np.int32),
                        n=np.zeros((P1, nd), np.int32), k=int(k), max_p=int(max_p))
    fs, keep = _host_struct(table)
    arrs = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (w0, w_min, w_max)]
    bg = HaldaBudgetC(ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), int(max_p))
    fr = HaldaFrontierC(nd, *(ptr(getattr(out, f)) for f in ("status", "obj", "moved", "w", "n")))
    m = model_struct(model, kv_factor)
    ctx.call("halda_solve_fleets_budget_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), int(k), ctypes.byref(bg),
             ctypes.byref(fr))
    del keep
    return out


def _flat(table: FleetTable, lists, fill: int) -> Optional[np.ndarray]:
    """Per-fleet int lists (None: no bound) in the table's device layout, None when no fleet has one."""
    if all(a is None for a in lists):
        return None
    out = np.full(table.n_devices, fill, np.int32)
    for f, a in enumerate(lists):
        if a is not None:
            o = int(table.dev_off[f])
            out[o:o + len(a)] = np.clip(a, -INT32_MAX, INT32_MAX)
    return out


def halda_move_frontier_batch(fleets: Sequence[Sequence[DeviceProfile]], model: ModelProfile,
                              incumbents: Sequence[Incumbent], max_moved_layers: int, kv_bits: str = "8bit",
                              w_min: Optional[Sequence[Optional[Sequence[int]]]] = None,
                              w_max: Optional[Sequence[Optional[Sequence[int]]]] = None,
                              device: int = 0) -> List[List[FrontierPoint]]:
    """Per fleet the move frontier around its incumbent: one FrontierPoint per p = 0 .. max_moved_layers // 2.
    One fleet table and one GPU call per distinct incumbent k, then one evaluation call that prices the incumbents
    (for `regret`) and every returned plan (obj_value formed on the host, as halda_evaluate_plan forms it).
    w_min / w_max: per fleet a list of per-device bounds or None. ValueError before any GPU work for a missing
    or malformed incumbent, a bad budget, or a shape outside the launch's gate (fleets of more than 64 devices,
    max_moved_layers // 2 > 63, an LDS slice beyond 160 KiB)."""
    kv_factor = kv_bits_to_factor(kv_bits)
    fleets = [list(d) for d in fleets]
    P = check_budget(max_moved_layers)
    if len(incumbents) != len(fleets):
        raise ValueError(f"{len(incumbents)} incumbents for {len(fleets)} fleets")
    for name, b in (("w_min", w_min), ("w_max", w_max)):
        if b is not None and len(b) != len(fleets):
            raise ValueError(f"{len(b)} {name} entries for {len(fleets)} fleets")
    plans, los, his = [], [], []
    for f, devs in enumerate(fleets):
        plans.append(check_incumbent(incumbents[f], len(devs), int(model.L)))
        lo, hi = check_bounds(None if w_min is None else w_min[f], None if w_max is None else w_max[f], len(devs))
        los.append(lo)
        his.append(hi)
    if not fleets:
        return []
    by_k = {}
    for f, p in enumerate(plans):
        by_k.setdefault(p[0], []).append(f)
    for k, fs in by_k.items():
        sizes = [len(fleets[f]) for f in fs]
        check_gate(max(sizes), min(sizes), P, k)
    raw: list = [None] * len(fleets)  # fleet -> [(w, n, moved) or None per point]
    for k, fs in sorted(by_k.items()):
        table = fleet_table([fleets[f] for f in fs], model)
        w0 = np.concatenate([np.asarray(plans[f][1], np.int32) for f in fs])
        res = solve_budget_table(table, model, k, w0, P, kv_factor, _flat(table, [los[f] for f in fs], 0),
                                 _flat(table, [his[f] for f in fs], INT32_MAX), device)
        for j, f in enumerate(fs):
            a, b = int(table.dev_off[j]), int(table.dev_off[j + 1])
            raw[f] = [([int(v) for v in res.w[p, a:b]], [int(v) for v in res.n[p, a:b]], int(res.moved[j, p]))
                      if int(res.status[j, p]) == STATUS_OPTIMAL else None for p in range(P + 1)]
    # obj_value = c.x + sum t_comm + sum xi + kappa formed on the host as every entry of this package forms it:
    # the incumbents and every distinct returned plan priced in ONE evaluation call (so a point's obj_value is
    # halda_evaluate_plan's of its plan, bit for bit)
    need = distinct_plans(raw)
    ev = halda_evaluate_plans_batch(fleets + [fleets[f] for f, _ in need], model,
                                    plans + [(plans[f][0], *raw[f][p][:2]) for f, p in need], kv_bits, device)
    rows = host_frontier(raw, need, [e.obj_value for e in ev[len(fleets):]])
    out = []
    for f, row in enumerate(rows):
        inc, k, sets, pts = ev[f], plans[f][0], assign_sets(fleets[f]), []
        for p, c in enumerate(row):
            if c is None:
                pts.append(FrontierPoint(2 * p, None, math.inf, 0, -math.inf if inc.feasible else math.inf))
                continue
            (w, n, moved), obj = c
            plan = HALDAResult(w=w, n=n, k=k, obj_value=obj, sets=sets)
            pts.append(FrontierPoint(2 * p, plan, obj, moved, inc.obj_value - obj if inc.feasible else math.inf))
        out.append(pts)
    return out


def halda_move_frontier(devs: Sequence[DeviceProfile], model: ModelProfile, incumbent: Incumbent,
                        max_moved_layers: int, kv_bits: str = "8bit", w_min: Optional[Sequence[int]] = None,
                        w_max: Optional[Sequence[int]] = None, device: int = 0) -> List[FrontierPoint]:
    """halda_move_frontier_batch for one fleet: the best plan at the incumbent's k for every budget
    0, 2, .. 2 (max_moved_layers // 2) of moved layers, in one GPU solve."""
    return halda_move_frontier_batch([list(devs)], model, [incumbent], max_moved_layers, kv_bits,
                                     None if w_min is None else [w_min], None if w_max is None else [w_max],
                                     device)[0]


def halda_solve_budget(devs: Sequence[DeviceProfile], model: ModelProfile, incumbent: Incumbent,
                       max_moved_layers: int, kv_bits: str = "8bit", w_min: Optional[Sequence[int]] = None,
                       w_max: Optional[Sequence[int]] = None, device: int = 0) -> HALDAResult:
    """The best plan at the incumbent's k that moves at most max_moved_layers layers in total (the frontier's
    last point); RuntimeError, as halda_solve raises it, when no plan lies within the budget and the bounds."""
    r = halda_move_frontier(devs, model, incumbent, max_moved_layers, kv_bits, w_min, w_max, device)[-1].plan
    if r is None:
        raise RuntimeError("No feasible MILP found within the move budget.")
    return r
