"""The k-sweep within per-device layer bounds (libhalda `halda_solve_fleets_bounded`): caps, pins, bounded moves.

`halda_replace_or_keep` reports how many layers the new optimum would move, but the caller cannot limit it.
Here the caller narrows the bounds of the `w` columns of every fixed-k MILP from `[1, W]` to
`[max(1, w_min_i), min(W, w_max_i)]`: "at most D layers per device away from the running plan"
(`move_bounds`, `halda_replace_within`), "device 3 takes at most 6 layers" (a cap), "devices 0 and 1 stay as
they are" (a pin, `w_min_i = w_max_i`). Everything else of the MILP is unchanged: the other devices' n are
re-optimised.

The GPU share n_i of those layers has a box of its own (libhalda `halda_solve_fleets_boxed`): `n_min` / `n_max`
narrow the n columns from the reference's `[0, nhi_i]` (nhi_i = W on a GPU device, else 0) to
`[max(0, n_min_i), min(nhi_i, n_max_i)]` -- "do not use this machine's GPU" (`n_max_i = 0`), "at most D layers
per device may change between RAM and VRAM" (`move_box`, `halda_replace_within(max_move_n=D)`), "pin what is
running" (both columns pinned: the answer prices that plan, as `halda_evaluate_plan` does). The link row
n_i <= w_i stays, so `n_min_i` is also a lower bound on w_i; every row, slack, z and C are the reference's.
A negative `n_min_i` means no bound; a crossing pair, or `n_min_i >= 1` on a device without a GPU, is simply
infeasible. An entry that gets no n bounds calls exactly what it called before they existed.
"""

from __future__ import annotations

import ctypes
import math
import numbers
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._abi import HaldaBoundsC, HaldaBoxC, HaldaFleetResultC
from ._libhalda import ROUTES, failure, get_context, last_route, ptr, set_path
from .coefficients import HALDAResult
from .fleets import FleetSolve, FleetTable, _host_struct, fleet_table, model_struct, open_x_offsets
from .halda import _batch_k_list, _batch_results, _positive_ks
from .lower import kv_bits_to_factor
from .plans import Incumbent, PlanEvaluation, _as_plan, halda_replace_or_keep_batch

INT32_MAX = 2**31 - 1
# (w_min, w_max) or (w_min, w_max, n_min, n_max), every entry a sequence of ints or None; None: no bounds
Bounds = Optional[Tuple[Optional[Sequence[int]], ...]]


BOUNDS_ROUTES = ROUTES["bounds"]  # halda_last_bounds_route's values 0 .. 3
_ROUTE_PATH = {"auto": None, "general": 1, "tables": 3}  # the `route` keyword -> halda_set_bounds_path


def set_bounds_path(ctx, path: int) -> None:
    """halda_set_bounds_path on a HaldaContext: 0 automatic, 1 always the general route, 2 the fused launch
    where it applies, 3 the fused launch where it applies, else the table launch
    (halda_sweep_bounds_tables_kernel: fleets of 1 .. 64 devices, any k, one launch) where that applies."""
    set_path(ctx, "bounds", path)


def check_route(route) -> Optional[int]:
    """The bounds path a `route` keyword selects for one call: None for "auto" (the context's path stays as it
    is), 1 for "general", 3 for "tables" (the fused launch, else the table launch, else general). ValueError
    for anything else."""
    if not isinstance(route, str) or route not in _ROUTE_PATH:
        raise ValueError(f"route: {route!r} is not one of {sorted(_ROUTE_PATH)}")
    return _ROUTE_PATH[route]


def last_bounds_route(ctx) -> str:
    """The route of the context's last halda_solve_fleets_bounded call: "fused", "general", "tables" or
    "none"."""
    return last_route(ctx, "bounds")


_NO_N = object()  # check_bounds' "called without the n arguments": the 2-tuple answer, as before they existed


def _int_list(a, what: str, M: int) -> List[int]:
    try:
        a = list(a)
    except TypeError:
        raise ValueError(f"{what}: {a!r} is neither an integer nor a sequence of integers") from None
    if len(a) != M:
        raise ValueError(f"{what} of {len(a)} entries for a fleet of {M} devices")
    for v in a:
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f"{what}: {v!r} is not an integer")
    return [int(v) for v in a]


def check_bounds(w_min, w_max, M: int, n_min=_NO_N, n_max=_NO_N):
    """(w_min, w_max) as int lists (None: no bound on that side). ValueError for a wrong length, a non-integer
    entry or w_min_i < 1; w_max_i < w_min_i is not an error (the instance is infeasible). With n_min / n_max
    given (a sequence or None each): (w_min, w_max, n_min, n_max), the n lists checked for length and integer
    entries alone -- a negative n_min_i means no bound and a crossing pair is infeasible, neither an error."""
    lo = None if w_min is None else _int_list(w_min, "w_min", M)
    hi = None if w_max is None else _int_list(w_max, "w_max", M)
    if lo is not None and any(v < 1 for v in lo):
        raise ValueError("w_min: every entry must be >= 1")
    if n_min is _NO_N and n_max is _NO_N:
        return lo, hi
    nlo = None if n_min is _NO_N or n_min is None else _int_list(n_min, "n_min", M)
    nhi = None if n_max is _NO_N or n_max is None else _int_list(n_max, "n_max", M)
    return lo, hi, nlo, nhi


def _check_entry(b, M: int):
    """One fleet's `bounds[f]` checked: a 2-tuple as check_bounds(w_min, w_max), a 4-tuple with the n lists."""
    try:
        n = len(b)
    except TypeError:
        raise ValueError(f"bounds entry {b!r} is neither None, (w_min, w_max) nor (w_min, w_max, n_min, n_max)") from None
    if n == 2:
        return check_bounds(b[0], b[1], M)
    if n == 4:
        return check_bounds(b[0], b[1], M, b[2], b[3])
    raise ValueError(f"bounds entry of {n} items: expected (w_min, w_max) or (w_min, w_max, n_min, n_max)")


def move_box(w0: Sequence[int], n0: Sequence[int], max_move: Union[int, Sequence[int]],
             max_move_n: Union[None, int, Sequence[int]] = None):
    """(w_min, w_max, n_min, n_max): move_bounds(w0, max_move) and, with max_move_n = Dn (an int or one per
    device), the n box (max(0, n0 - Dn), n0 + Dn). max_move_n=None leaves n free: n_min = n_max = None."""
    w_min, w_max = move_bounds(w0, max_move)
    n0 = _int_list(n0, "n0", len(w_min))
    if max_move_n is None:
        return w_min, w_max, None, None
    if isinstance(max_move_n, numbers.Integral) and not isinstance(max_move_n, bool):
        D = [int(max_move_n)] * len(n0)
    else:
        D = _int_list(max_move_n, "max_move_n", len(n0))
    if any(d < 0 for d in D):
        raise ValueError("max_move_n must be >= 0")
    return w_min, w_max, [max(0, n - d) for n, d in zip(n0, D)], [n + d for n, d in zip(n0, D)]


def move_bounds(w0: Sequence[int], max_move: Union[int, Sequence[int]]) -> Tuple[List[int], List[int]]:
    """The box of plans at most `max_move` layers per device away from w0: (max(1, w0 - D), w0 + D), D an int
    or one per device."""
    w0 = _int_list(w0, "w0", len(list(w0)))
    if isinstance(max_move, numbers.Integral) and not isinstance(max_move, bool):
        D = [int(max_move)] * len(w0)
    else:
        D = _int_list(max_move, "max_move", len(w0))
    if any(d < 0 for d in D):
        raise ValueError("max_move must be >= 0")
    return [max(1, w - d) for w, d in zip(w0, D)], [w + d for w, d in zip(w0, D)]


def bounds_arrays(table: FleetTable, bounds: Sequence[Bounds]):
    """(w_min, w_max) int32 in the table's device layout: 0 / INT32_MAX ("no bound") where a fleet has none;
    entries beyond the int32 range are clipped to it (they bind no more than the range's ends). Where some
    fleet's entry is a 4-tuple with an n list: (w_min, w_max, n_min, n_max), the n arrays in the same layout
    and with the same "no bound" values (a negative n_min_i is written as 0)."""
    nf, nd = table.n_fleets, table.n_devices
    if len(bounds) != nf:
        raise ValueError(f"{len(bounds)} bounds for {nf} fleets")
    lo, hi = np.zeros(nd, np.int32), np.full(nd, INT32_MAX, np.int32)
    nlo = nhi = None
    sizes = table.sizes()
    for f, b in enumerate(bounds):
        if b is None:
            continue
        got = _check_entry(b, int(sizes[f]))
        w_min, w_max = got[0], got[1]
        a = int(table.dev_off[f])
        if w_min is not None:
            lo[a:a + len(w_min)] = np.clip(w_min, 0, INT32_MAX)
        if w_max is not None:
            hi[a:a + len(w_max)] = np.clip(w_max, -INT32_MAX, INT32_MAX)
        if len(got) == 4 and (got[2] is not None or got[3] is not None):
            if nlo is None:
                nlo, nhi = np.zeros(nd, np.int32), np.full(nd, INT32_MAX, np.int32)
            if got[2] is not None:
                nlo[a:a + len(got[2])] = np.clip(got[2], 0, INT32_MAX)
            if got[3] is not None:
                nhi[a:a + len(got[3])] = np.clip(got[3], -INT32_MAX, INT32_MAX)
    return (lo, hi) if nlo is None else (lo, hi, nlo, nhi)


def solve_bounded_table(table: FleetTable, model: ModelProfile, pos: List[int], w_min: Optional[np.ndarray],
                        w_max: Optional[np.ndarray], kv_factor: float, device: int = 0,
                        route: str = "auto", n_min: Optional[np.ndarray] = None,
                        n_max: Optional[np.ndarray] = None) -> FleetSolve:
    """One halda_solve_fleets_bounded_host call on a packed table: the bounded sweep's FleetSolve
    (want_x="open"). `route`: "auto" follows the context's bounds path; "general" / "tables" set it for this
    call alone (inside the context's lock) and put the previous one back. With n_min or n_max the call is
    halda_solve_fleets_boxed_host."""
    path = check_route(route)
    ctx = get_context(device)
    nf, nd, nk = table.n_fleets, table.n_devices, len(pos)
    xsel = open_x_offsets(table, model, pos)
    ext = int(np.max(xsel + np.repeat(7 * table.sizes() + 1, nk), initial=0)) if (xsel >= 0).any() else 0
    fbuf, ibuf = np.zeros(nf + nf * nk + 2 * ext), np.zeros(nf + 2 * nd + nf * nk, np.int32)
    pf, pi = fbuf.ctypes.data, ibuf.ctypes.data
    o1, o2 = nf, nf + nf * nk
    out = FleetSolve(best_k=ibuf[:nf], obj_value=fbuf[:nf], w=ibuf[nf:nf + nd], n=ibuf[nf + nd:nf + 2 * nd],
                     obj_by_k=fbuf[o1:o2].reshape(nf, nk), status=ibuf[nf + 2 * nd:].reshape(nf, nk), ks=pos,
                     x=fbuf[o2:o2 + ext], c=fbuf[o2 + ext:], x_off=xsel)
    r = HaldaFleetResultC(pi, pf, pi + 4 * nf, pi + 4 * (nf + nd), pf + 8 * o1, pi + 4 * (nf + 2 * nd), pf + 8 * o2,
                          pf + 8 * (o2 + ext), xsel.ctypes.data)
    fs, keep = _host_struct(table)
    lo = None if w_min is None else np.ascontiguousarray(w_min, np.int32)
    hi = None if w_max is None else np.ascontiguousarray(w_max, np.int32)
    boxed = n_min is not None or n_max is not None
    nlo = None if n_min is None else np.ascontiguousarray(n_min, np.int32)
    nhi = None if n_max is None else np.ascontiguousarray(n_max, np.int32)
    bd = HaldaBoxC(ptr(lo), ptr(hi), ptr(nlo), ptr(nhi)) if boxed else HaldaBoundsC(ptr(lo), ptr(hi))
    name = "halda_solve_fleets_boxed_host" if boxed else "halda_solve_fleets_bounded_host"
    karr = np.asarray(pos, np.int32)
    m = model_struct(model, kv_factor)
    with ctx._lock:
        prev = ctx.paths.get("bounds", 0)  # (the library has no getter)
        if path is not None:
            set_path(ctx, "bounds", path)
        try:
            rc = getattr(ctx.lib, name)(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), karr.ctypes.data, nk,
                                        ctypes.byref(bd), ctypes.byref(r))
        finally:
            if path is not None:
                set_path(ctx, "bounds", prev)
    del keep
    if rc != 0:  # (checked once the path is back and the lock released)
        raise failure(ctx.lib, name, rc)
    return out


def halda_solve_bounded_batch(fleets: Sequence[Sequence[DeviceProfile]], model: ModelProfile,
                              bounds: Sequence[Bounds], k_candidates: Optional[Iterable[int]] = None,
                              kv_bits: str = "8bit", device: int = 0,
                              route: str = "auto") -> List[Optional[HALDAResult]]:
    """Many fleets, each within its own bounds (`bounds[f]` = (w_min, w_max) or (w_min, w_max, n_min, n_max),
    any of them None, or None for no bounds), in ONE GPU call (halda_solve_fleets_boxed_host where some fleet
    has an n list, else halda_solve_fleets_bounded_host). One HALDAResult per fleet, None where no k is feasible within the bounds.
    `route`: "auto" (the context's bounds path), "general", or "tables" -- one table launch for small fleets
    and k > 1 where the fused launch does not apply (at most 64 devices per fleet; general elsewhere)."""
    check_route(route)
    kv_factor = kv_bits_to_factor(kv_bits)
    fleets = fleets if isinstance(fleets, (list, tuple)) else list(fleets)
    if len(bounds) != len(fleets):
        raise ValueError(f"{len(bounds)} bounds for {len(fleets)} fleets")
    for devs, b in zip(fleets, bounds):  # the argument errors before any packing or GPU call
        if b is not None:
            _check_entry(b, len(devs))
    if k_candidates is not None and not isinstance(k_candidates, (list, tuple)):
        k_candidates = list(k_candidates)
    Ks = _batch_k_list(model, k_candidates)
    if not fleets:
        return []
    if not Ks:
        return [None] * len(fleets)
    pos = _positive_ks(Ks)
    table = fleet_table(fleets, model)
    if not pos:
        return [None] * len(fleets)
    arrs = bounds_arrays(table, bounds)
    res = solve_bounded_table(table, model, pos, arrs[0], arrs[1], kv_factor, device, route, *arrs[2:])
    return _batch_results(table, res, pos, model)


def halda_solve_bounded(devs: Sequence[DeviceProfile], model: ModelProfile, w_min: Optional[Sequence[int]] = None,
                        w_max: Optional[Sequence[int]] = None, k_candidates: Optional[Iterable[int]] = None,
                        kv_bits: str = "8bit", device: int = 0, route: str = "auto",
                        n_min: Optional[Sequence[int]] = None, n_max: Optional[Sequence[int]] = None) -> HALDAResult:
    """halda_solve with every device's layer count kept in [w_min_i, w_max_i] and, with n_min / n_max, its GPU
    share in [n_min_i, n_max_i]; RuntimeError, as halda_solve raises it, when no k is feasible within the
    bounds. `route`: as halda_solve_bounded_batch."""
    check_route(route)
    devs = list(devs)
    if n_min is not None or n_max is not None:
        b = (w_min, w_max, n_min, n_max)
    else:
        b = None if w_min is None and w_max is None else (w_min, w_max)
    r = halda_solve_bounded_batch([devs], model, [b], k_candidates, kv_bits, device, route)[0]
    if r is None:
        raise RuntimeError("No feasible MILP found for any k this round.")
    return r


@dataclass(frozen=True)
class ReplacementWithin:
    """halda_replace_within's answer: halda_replace_or_keep's fields, and `within` -- the best plan at the
    incumbent's k at most max_move layers per device away from it (None where the box holds no plan) --
    with regret_within = incumbent.obj_value - within.obj_value, moved_layers_within and
    gap_to_free = within.obj_value - best.obj_value (what the move budget costs; inf without `within`).
    moved_gpu_layers_within = sum |n_i - n0_i| of `within` against the incumbent (0 without `within`)."""

    incumbent: PlanEvaluation
    best: Optional[HALDAResult]
    regret: float
    moved_layers: int
    replace: bool
    within: Optional[HALDAResult]
    regret_within: float
    moved_layers_within: int
    gap_to_free: float
    moved_gpu_layers_within: int = 0


def halda_replace_within_batch(fleets: Sequence[Sequence[DeviceProfile]], model: ModelProfile,
                               incumbents: Sequence[Incumbent], max_move: Union[int, Sequence[int]],
                               kv_bits: str = "8bit", rel_tol: float = 0.0, device: int = 0,
                               route: str = "auto",
                               max_move_n: Union[None, int, Sequence[int]] = None) -> List[ReplacementWithin]:
    """Per fleet: halda_replace_or_keep (the incumbent priced, the free optimum), then the best plan inside
    the move box around the incumbent at the incumbent's k -- one bounded call per distinct incumbent k.
    `route`: the bounded calls' route, as halda_solve_bounded_batch ("tables" is the one for an incumbent at
    k > 1 or a small fleet). With max_move_n, `within` is the best plan at the incumbent's k inside both
    boxes: at most max_move layers per device moved between devices AND at most max_move_n of a device's
    layers moved between RAM and VRAM."""
    check_route(route)
    fleets = fleets if isinstance(fleets, (list, tuple)) else list(fleets)
    base = halda_replace_or_keep_batch(fleets, model, incumbents, rel_tol, kv_bits, None, device)
    plans = [_as_plan(p) for p in incumbents]
    within: List[Optional[HALDAResult]] = [None] * len(fleets)
    by_k = {}
    for f, p in enumerate(plans):
        if p is not None:
            by_k.setdefault(int(p[0]), []).append(f)
    for k, fs in sorted(by_k.items()):
        if max_move_n is None:
            boxes = [move_bounds(plans[f][1], max_move) for f in fs]
        else:
            boxes = [move_box(plans[f][1], plans[f][2], max_move, max_move_n) for f in fs]
        got = halda_solve_bounded_batch([fleets[f] for f in fs], model, boxes, [k], kv_bits, device, route)
        for f, r in zip(fs, got):
            within[f] = r
    out = []
    for b, p, wi in zip(base, plans, within):
        moved = 0 if wi is None or p is None else int(sum(abs(int(a) - int(c)) for a, c in zip(wi.w, p[1])))
        moved_n = 0 if wi is None or p is None else int(sum(abs(int(a) - int(c)) for a, c in zip(wi.n, p[2])))
        if wi is None:
            rw = -math.inf if b.incumbent.feasible else math.inf
        else:
            rw = b.incumbent.obj_value - wi.obj_value if b.incumbent.feasible else math.inf
        gap = math.inf if wi is None or b.best is None else wi.obj_value - b.best.obj_value
        out.append(ReplacementWithin(b.incumbent, b.best, b.regret, b.moved_layers, b.replace, wi, rw, moved, gap,
                                     moved_n))
    return out


def halda_replace_within(devs: Sequence[DeviceProfile], model: ModelProfile, incumbent: Incumbent,
                         max_move: Union[int, Sequence[int]], kv_bits: str = "8bit", rel_tol: float = 0.0,
                         device: int = 0, route: str = "auto",
                         max_move_n: Union[None, int, Sequence[int]] = None) -> ReplacementWithin:
    """halda_replace_within_batch for one fleet."""
    check_route(route)
    return halda_replace_within_batch([list(devs)], model, [incumbent], max_move, kv_bits, rel_tol, device,
                                      route, max_move_n)[0]
