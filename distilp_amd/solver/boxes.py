"""One fleet table under many boxes in one GPU call (libhalda `halda_solve_fleets_boxes`), and the reload-time
frontier built on it.

`halda_solve_bounded_batch` takes one box per fleet, so a ladder of boxes on ONE fleet -- +-D for several D, "cap
this machine at c layers" for several c, a set of "CPU only on device i" what-ifs -- had to materialise the
fleet once per box: that many packings and that many tables over PCIe. Here the fleets are packed once and every
box is a plane of the four bound arrays: `boxes[b]` is what `halda_solve_bounded_batch` takes as `bounds`, and
`out[b]` is what it returns for it with route="tables", bit for bit.

The reload frontier is the ladder an operator asks for after a re-profile. A device that gains layers reads them
from its own disk and the devices do so in parallel, so a re-placement costs max_i gained_i * k * b_layer /
s_disk_i seconds of outage. "The best plan I can reach in T seconds" is, for one T, a per-device cap
w_max_i = w0_i + cap_i(T); over T it is a ladder of nested boxes (`reload_caps`), solved in one call
(`halda_reload_frontier`). Only layers that change DEVICE are priced: the n side is free, because a layer that
moves between RAM and VRAM on its own device reads no disk.
"""

from __future__ import annotations

import ctypes
import math
import numbers
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._abi import HaldaBoxesC, HaldaFleetResultC
from ._libhalda import get_context, last_route, ptr, set_path
from .bounds import INT32_MAX, Bounds, _check_entry
from .budget import check_incumbent
from .coefficients import HALDAResult
from .fleets import FleetSolve, FleetTable, _host_struct, fleet_constants, fleet_table, model_struct, open_x_offsets
from .halda import _batch_k_list, _batch_results, _positive_ks
from .lower import kv_bits_to_factor
from .plans import Incumbent
from .subfleets import ItemTable

MAX_BOXES = 65535  # halda_solve_fleets_boxes: blockIdx.y is the box

_NO_BOUND = (0, INT32_MAX, 0, INT32_MAX)  # w_min, w_max, n_min, n_max


def set_boxes_path(ctx, path: int) -> None:
    """halda_set_boxes_path on a HaldaContext: 0 automatic (default), 1 always loop (test path)."""
    set_path(ctx, "boxes", path)


def last_boxes_route(ctx) -> str:
    """The route of the context's last halda_solve_fleets_boxes call: "register", "tables", "loop" or "none"."""
    return last_route(ctx, "boxes")


def check_boxes(boxes, sizes: Sequence[int]) -> list:
    """`boxes` as a list of per-fleet entry lists, every entry None or what bounds._check_entry makes of it (int
    lists or None, by its rules). ValueError for an empty list, more than 65,535 boxes, a box that does not hold one
    entry per fleet, or a bad entry."""
    try:
        boxes = list(boxes)
    except TypeError:
        raise ValueError(f"boxes: {boxes!r} is not a sequence of boxes") from None
    if not boxes:
        raise ValueError("boxes is empty: at least one box is needed")
    if len(boxes) > MAX_BOXES:
        raise ValueError(f"{len(boxes)} boxes: at most {MAX_BOXES} in one call")
    out = []
    for b, box in enumerate(boxes):
        try:
            box = list(box)
        except TypeError:
            raise ValueError(f"box {b}: {box!r} is not a sequence of one bounds entry per fleet") from None
        if len(box) != len(sizes):
            raise ValueError(f"box {b}: {len(box)} bounds for {len(sizes)} fleets")
        out.append([None if e is None else _check_entry(e, int(M)) for e, M in zip(box, sizes)])
    return out


def box_planes(table: FleetTable, boxes: Sequence[Sequence[Bounds]], checked: bool = False) -> tuple:
    """(w_min, w_max, n_min, n_max) of halda_boxes: int32 [n_box, n_devices], box b's row what bounds_arrays makes
    of boxes[b] ("no bound" is 0 / INT32_MAX, entries beyond the int32 range are clipped to it, a negative n_min is
    written as 0). The n planes are None unless some box has an n list. checked: `boxes` is check_boxes' result."""
    sizes = table.sizes()
    if not checked:
        boxes = check_boxes(boxes, sizes)
    nb, nd = len(boxes), table.n_devices
    boxed = any(e is not None and len(e) == 4 and (e[2] is not None or e[3] is not None) for box in boxes for e in box)
    planes = [np.full((nb, nd), _NO_BOUND[a], np.int32) for a in range(4 if boxed else 2)]
    floor = (0, -INT32_MAX, 0, -INT32_MAX)
    off = [int(v) for v in table.dev_off]
    for f in range(table.n_fleets):  # one conversion per (array, fleet): the lists of every box that has one
        for a in range(len(planes)):
            rows = [(b, box[f][a]) for b, box in enumerate(boxes)
                    if box[f] is not None and a < len(box[f]) and box[f][a] is not None]
            if rows:
                planes[a][[b for b, _ in rows], off[f]:off[f + 1]] = np.clip([v for _, v in rows], floor[a], INT32_MAX)
    return tuple(planes) if boxed else (*planes, None, None)


def _solve_planes(table: FleetTable, model: ModelProfile, pos: List[int], planes, kv_factor: float,
                  device: int) -> Tuple[FleetSolve, int, int]:
    """One halda_solve_fleets_boxes_host call: (the FleetSolve of all n_box * n_fleets (box, fleet) rows, box-major,
    with the call's compact x / c layout -- box b's rows moved by b * ext elements --, n_box, ext)."""
    planes = [None if p is None else np.ascontiguousarray(p, np.int32) for p in planes]
    if len(planes) != 4:
        raise ValueError(f"planes: {len(planes)} arrays, expected (w_min, w_max, n_min, n_max)")
    nf, nd, nk = table.n_fleets, table.n_devices, len(pos)
    shapes = {p.shape for p in planes if p is not None}
    if not shapes:
        raise ValueError("planes: every array is None, the number of boxes is unknown")
    if len(shapes) != 1 or len(next(iter(shapes))) != 2 or next(iter(shapes))[1] != nd:
        raise ValueError(f"planes: shapes {sorted(shapes)}, expected one [n_box, {nd}]")
    nb = int(next(iter(shapes))[0])
    if nb < 1 or nb > MAX_BOXES:
        raise ValueError(f"{nb} boxes: 1 .. {MAX_BOXES} in one call")
    ctx = get_context(device)
    xsel = open_x_offsets(table, model, pos)
    ext = int(np.max(xsel + np.repeat(7 * table.sizes() + 1, nk), initial=0)) if (xsel >= 0).any() else 0
    base = (np.arange(nb, dtype=np.int64) * ext)[:, None]
    xall = np.where(xsel[None, :] >= 0, xsel[None, :] + base, -1).astype(np.int64).ravel()
    # f64: obj_value | obj_by_k | x | c; int32: best_k | w | n | status -- each box-major
    fbuf, ibuf = np.zeros(nb * (nf + nf * nk + 2 * ext)), np.zeros(nb * (nf + 2 * nd + nf * nk), np.int32)
    f_obk, f_x, f_c = nb * nf, nb * (nf + nf * nk), nb * (nf + nf * nk + ext)
    i_w, i_n, i_st = nb * nf, nb * (nf + nd), nb * (nf + 2 * nd)
    res = FleetSolve(best_k=ibuf[:i_w], obj_value=fbuf[:f_obk], w=ibuf[i_w:i_n], n=ibuf[i_n:i_st],
                     obj_by_k=fbuf[f_obk:f_x].reshape(nb * nf, nk), status=ibuf[i_st:].reshape(nb * nf, nk), ks=pos,
                     x=fbuf[f_x:f_c], c=fbuf[f_c:], x_off=xall)
    r = HaldaFleetResultC(*(ptr(a) for a in (res.best_k, res.obj_value, res.w, res.n, res.obj_by_k, res.status, res.x,
                                             res.c, xall)))
    fs, keep = _host_struct(table)
    bx = HaldaBoxesC(nb, *(ptr(p) for p in planes))
    karr = np.asarray(pos, np.int32)
    m = model_struct(model, kv_factor)
    ctx.call("halda_solve_fleets_boxes_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), karr.ctypes.data, nk,
             ctypes.byref(bx), ctypes.byref(r))
    del keep
    return res, nb, ext


def solve_boxes_table(table: FleetTable, model: ModelProfile, pos: List[int], planes, kv_factor: float,
                      device: int = 0) -> List[FleetSolve]:
    """One halda_solve_fleets_boxes_host call on a packed table. `planes` = (w_min, w_max, n_min, n_max), each
    int32 [n_box, n_devices] or None (no bound on that side in any box). Per box the FleetSolve
    (want_x="open") of its slice: views of one result buffer, with the box's x / c rows from 0 and the per-table
    x_off."""
    res, nb, ext = _solve_planes(table, model, pos, planes, kv_factor, device)
    nf, nd = table.n_fleets, table.n_devices
    xsel = res.x_off[:nf * len(pos)]  # box 0's offsets are the table's own
    return [FleetSolve(best_k=res.best_k[b * nf:(b + 1) * nf], obj_value=res.obj_value[b * nf:(b + 1) * nf],
                       w=res.w[b * nd:(b + 1) * nd], n=res.n[b * nd:(b + 1) * nd],
                       obj_by_k=res.obj_by_k[b * nf:(b + 1) * nf], status=res.status[b * nf:(b + 1) * nf], ks=pos,
                       x=res.x[b * ext:(b + 1) * ext], c=res.c[b * ext:(b + 1) * ext], x_off=xsel) for b in range(nb)]


def halda_solve_boxes_batch(fleets: Sequence[Sequence[DeviceProfile]], model: ModelProfile,
                            boxes: Sequence[Sequence[Bounds]], k_candidates: Optional[Iterable[int]] = None,
                            kv_bits: str = "8bit", device: int = 0) -> List[List[Optional[HALDAResult]]]:
    """Many fleets under many boxes, the fleets packed once and every box in ONE GPU call
    (halda_solve_fleets_boxes_host). `boxes[b]` is what halda_solve_bounded_batch takes as `bounds`: one entry
    per fleet, each None, (w_min, w_max) or (w_min, w_max, n_min, n_max). out[b][f] is a HALDAResult, or None
    where no k is feasible inside box b, and equals
    halda_solve_bounded_batch(fleets, model, boxes[b], k_candidates, kv_bits, route="tables")[f] bit for bit.
    ValueError before any packing or GPU work for an empty box list, more than 65,535 boxes, a box without one
    entry per fleet, or a bad entry (bounds._check_entry's rules)."""
    kv_factor = kv_bits_to_factor(kv_bits)
    fleets = fleets if isinstance(fleets, (list, tuple)) else list(fleets)
    boxes = check_boxes(boxes, [len(d) for d in fleets])
    if k_candidates is not None and not isinstance(k_candidates, (list, tuple)):
        k_candidates = list(k_candidates)
    Ks = _batch_k_list(model, k_candidates)
    if not fleets:
        return [[] for _ in boxes]
    if not Ks:
        return [[None] * len(fleets) for _ in boxes]
    pos = _positive_ks(Ks)
    table = fleet_table(fleets, model)
    if not pos:
        return [[None] * len(fleets) for _ in boxes]
    res, nb, _ = _solve_planes(table, model, pos, box_planes(table, boxes, checked=True), kv_factor, device)
    # the (box, fleet) rows seen as n_box * n_fleets fleets: the table's extents, classes and constants once per box
    nf, nd = table.n_fleets, table.n_devices
    off = (table.dev_off[None, :-1] + nd * np.arange(nb, dtype=np.int64)[:, None]).ravel()
    rows = ItemTable(np.append(off, nb * nd), np.tile(table.os_class, nb), None,
                     tuple(np.tile(c, nb) for c in fleet_constants(table, model)))
    flat = _batch_results(rows, res, pos, model, consts=rows.consts)
    return [flat[b * nf:(b + 1) * nf] for b in range(nb)]


def halda_solve_boxes(devs: Sequence[DeviceProfile], model: ModelProfile, boxes: Sequence[Bounds],
                      k_candidates: Optional[Iterable[int]] = None, kv_bits: str = "8bit",
                      device: int = 0) -> List[Optional[HALDAResult]]:
    """halda_solve_boxes_batch for one fleet: `boxes[b]` is None, (w_min, w_max) or (w_min, w_max, n_min, n_max);
    out[b] is the best plan inside box b, None where it holds none."""
    try:
        boxes = [[b] for b in boxes]
    except TypeError:
        raise ValueError(f"boxes: {boxes!r} is not a sequence of boxes") from None
    return [r[0] for r in halda_solve_boxes_batch([list(devs)], model, boxes, k_candidates, kv_bits, device)]


def reload_caps(w0: Sequence[int], s_disk: Sequence[float], W: int, max_points: int = 256,
                max_seconds_per_layer: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The breakpoints of "how many layers may device i gain in t seconds per layer-byte", and the caps at each.

    Device i of M may gain m = 1 .. W - (M - 1) - w0_i layers (every other device keeps at least one), and m
    layers take t(i, m) = m / s_disk_i -- one FP64 division. Returns (t, caps): t float64 [J], t[0] = 0 followed
    by the distinct t(i, m) in ascending order (equal quotients on two devices are one point); caps int64 [J, M],
    caps[j][i] = #{m : t(i, m) <= t[j]}, counted on those same quotients -- never floor(t * s_disk), which can
    disagree with the breakpoint by rounding. caps[0] = 0 and caps is non-decreasing along j. The list is cut
    after max_points points (t = 0 included) and before the first t > max_seconds_per_layer. Pure NumPy.
    Multiply t by the bytes of a layer group, k * b_layer, for seconds."""
    if isinstance(W, bool) or not isinstance(W, numbers.Integral):
        raise ValueError(f"W: {W!r} is not an integer")
    if isinstance(max_points, bool) or not isinstance(max_points, numbers.Integral) or max_points < 1:
        raise ValueError(f"max_points: {max_points!r} is not a positive integer")
    w0 = [int(v) for v in w0]
    s = np.asarray(list(s_disk), np.float64)
    M = len(w0)
    if len(s) != M:
        raise ValueError(f"s_disk of {len(s)} entries for w0 of {M}")
    if M and not (np.isfinite(s).all() and (s > 0.0).all()):
        raise ValueError("s_disk: every entry must be positive and finite")
    if max_seconds_per_layer is not None and not max_seconds_per_layer >= 0.0:
        raise ValueError(f"max_seconds_per_layer: {max_seconds_per_layer!r} must be >= 0")
    quot = [np.arange(1, max(0, int(W) - (M - 1) - w0[i]) + 1, dtype=np.float64) / s[i] for i in range(M)]
    t = np.concatenate([np.zeros(1)] + quot)
    t = np.unique(t)  # ascending, distinct; 0 first (every quotient is > 0)
    if max_seconds_per_layer is not None:
        t = t[t <= max_seconds_per_layer]
    t = t[:int(max_points)]
    caps = np.zeros((len(t), M), np.int64)
    for i in range(M):
        caps[:, i] = np.searchsorted(quot[i], t, side="right")
    return t, caps


@dataclass(frozen=True)
class ReloadPoint:
    """Point j of a reload frontier: the outage budget `seconds`, the per-device gain caps it allows, the best
    plan within them (None where there is none), its obj_value (inf without a plan), the layers each device
    gains under it, gained_i = max(0, w_i - w0_i), the outage it really takes,
    seconds_used = max_i gained_i / s_disk_i * (k * b_layer) <= seconds, and regret = obj_value minus the
    unbounded optimum's at the same k (0 at the end of an uncut frontier; inf without a plan)."""

    seconds: float
    caps: List[int]
    plan: Optional[HALDAResult]
    obj_value: float
    gained: List[int]
    seconds_used: float
    regret: float


def halda_reload_frontier(devs: Sequence[DeviceProfile], model: ModelProfile, incumbent: Incumbent,
                          max_seconds: Optional[float] = None, max_points: int = 256, kv_bits: str = "8bit",
                          device: int = 0) -> List[ReloadPoint]:
    """The best plan reachable in T seconds of reload, for every T at which the answer can change.

    At the incumbent's k (W = L // k), point j is the optimum inside w_max = w0 + caps[j] of
    reload_caps(w0, s_disk, W, max_points, max_seconds / (k * b_layer)): no lower bound, because giving layers
    up costs no reload, and n free -- the n side is NOT priced: a layer that moves between RAM and VRAM on its
    own device reads no disk. Point 0 is "w pinned, n re-optimised"; with no cut the last point is the
    unbounded optimum at k. Every point and one unbounded box (the regret baseline) go in ONE halda_solve_boxes
    call. Along j a strict running minimum is taken on the host-formed objectives: a point that does not
    strictly improve keeps the previous point's plan (which its caps also admit), halda_move_frontier's rule.
    seconds = t[j] * (k * b_layer); seconds_used is formed from the same quotients gained_i / s_disk_i, so it
    never exceeds seconds by rounding. ValueError before any GPU work for a missing or malformed incumbent (as
    halda_move_frontier), a bad max_points or a negative max_seconds."""
    devs = list(devs)
    kv_bits_to_factor(kv_bits)
    k, w0, _ = check_incumbent(incumbent, len(devs), int(model.L))
    if isinstance(max_points, bool) or not isinstance(max_points, numbers.Integral) or not 1 <= max_points < MAX_BOXES:
        raise ValueError(f"max_points: {max_points!r} must be an integer in 1 .. {MAX_BOXES - 1}")
    if max_seconds is not None and not max_seconds >= 0.0:
        raise ValueError(f"max_seconds: {max_seconds!r} must be >= 0")
    group = float(k * int(model.b_layer))  # bytes of one layer group: what a gained layer reads from disk
    s_disk = [float(d.s_disk) for d in devs]
    t, caps = reload_caps(w0, s_disk, int(model.L) // k, max_points,
                          None if max_seconds is None else max_seconds / group)
    boxes: list = [(None, [a + int(c) for a, c in zip(w0, row)]) for row in caps]
    boxes.append(None)
    res = halda_solve_boxes(devs, model, boxes, [k], kv_bits, device)
    free = res[-1]
    out: List[ReloadPoint] = []
    best: Optional[HALDAResult] = None
    for j, r in enumerate(res[:-1]):
        if r is not None and (best is None or r.obj_value < best.obj_value):
            best = r
        gained = [0] * len(devs) if best is None else [max(0, int(a) - b) for a, b in zip(best.w, w0)]
        used = max((g / s for g, s in zip(gained, s_disk)), default=0.0) * group
        obj = math.inf if best is None else float(best.obj_value)
        regret = math.inf if best is None or free is None else obj - float(free.obj_value)
        out.append(ReloadPoint(float(t[j]) * group, [int(c) for c in caps[j]], best, obj, gained, used, regret))
    return out
