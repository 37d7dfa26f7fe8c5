"""Sub-fleets of a packed fleet table: leave-one-out and what-if (libhalda `halda_solve_subfleets`).

An item is (parent fleet f, index list s): the fleet `[fleets[f][j] for j in s]`, in that order -- kappa's
head is the first listed device with is_head, else the first listed device. Each parent's DeviceProfiles
are packed once (`fleet_table`); the items travel as three index arrays, and the GPU either gathers each
item's device fields straight from the parent table (one wave per item, lists of one length <= 64 whose
sweep needs no tables: leave-one-out of 64-device fleets) or first expands the listed devices into a
compact table in device scratch. Either way item i's result is exactly
`halda_solve_batch([[fleets[f][j] for j in s]], ...)[0]`: the per-item host constants, device classes and
kappa heads come straight from the packed parent table and the index arrays (`item_table`: the C packer's
`consts_items`, the loops of its `consts`), equal to those of `gather_table` -- the NumPy gather that is
array for array the table `fleet_table` makes of the materialised lists, kept as the specification and
the fallback -- and the objective is formed by halda.py's own `_batch_results` from the returned c and x.

The reference's errors arise as for the materialised lists: the parents' packing raises what every device
raises, and what only a list's own head raises -- a zero s_disk, a CPU FLOPs row without "b_1" that only
kappa reads -- is raised per item (`item_table`, `check_item_heads`).
"""

from __future__ import annotations

import ctypes
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._abi import BYTE_FIELDS, F64_FIELDS, HaldaFleetResultC, HaldaSubfleetsC
from ._libhalda import get_context, last_route, ptr, set_path
from .coefficients import HALDAResult
from .fleets import (_PACKER, DEV_CPU_RATE, DEV_HEAD, FleetSolve, FleetTable, _host_struct, _scratch,
                     fleet_constants, fleet_table, model_struct, open_x_offsets)
from .fleets import _bind as _bind_sub  # noqa: F401 -- the identity, for callers from before load_library bound all
from .halda import _batch_k_list, _batch_results, _positive_ks
from .lower import kv_bits_to_factor

# Most listed devices in one GPU call: the expansion route's table is the only memory of size
# O(sum of list lengths), 130 bytes per listed device (about 270 MB at the default).
SUBFLEET_CHUNK_DEVICES = 1 << 21


def set_subfleets_path(ctx, path: int) -> None:
    """halda_set_subfleets_path on a HaldaContext: 0 automatic (default), 1 always expand (test path)."""
    set_path(ctx, "subfleets", path)


def last_subfleets_route(ctx) -> str:
    """The route of the context's last halda_solve_subfleets call: "fused", "expand" or "none"."""
    return last_route(ctx, "subfleets")


def pack_items(sizes: np.ndarray, items: Sequence[Tuple[int, Sequence[int]]]):
    """(parent int32 [n], sub_off int64 [n + 1], sub_idx int32 [sub_off[n]]) of `items` over parents of
    `sizes` devices. IndexError for a parent or device index out of range, ValueError for an empty list."""
    parent = np.asarray([int(f) for f, _ in items], np.int64)
    lists = [np.asarray(s, np.int64).reshape(-1) for _, s in items]
    lens = np.asarray([len(s) for s in lists], np.int64)
    sub_off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum(lens, out=sub_off[1:])
    sub_idx = np.concatenate(lists) if lists else np.zeros(0, np.int64)
    check_items(sizes, parent, sub_off, sub_idx)
    return parent.astype(np.int32), sub_off, sub_idx.astype(np.int32)


def check_items(sizes: np.ndarray, parent: np.ndarray, sub_off: np.ndarray, sub_idx: np.ndarray) -> None:
    """The argument errors of an item list (what halda_solve_subfleets_host rejects with HALDA_E_ARG)."""
    nf = len(sizes)
    bad = np.flatnonzero((parent < 0) | (parent >= nf))
    if len(bad):
        i = int(bad[0])
        raise IndexError(f"item {i}: fleet index {int(parent[i])} out of range for {nf} fleets")
    lens = np.diff(sub_off)
    bad = np.flatnonzero(lens < 1)
    if len(bad):
        raise ValueError(f"item {int(bad[0])}: empty device list")
    m = np.repeat(np.asarray(sizes, np.int64)[parent], lens)
    bad = np.flatnonzero((sub_idx < 0) | (sub_idx >= m))
    if len(bad):
        e = int(bad[0])
        i = int(np.searchsorted(sub_off, e, side="right") - 1)
        raise IndexError(f"item {i}: device index {int(sub_idx[e])} out of range for a fleet of {int(m[e])} devices")


def plan_chunks(lens: Sequence[int], limit: int) -> List[Tuple[int, int]]:
    """Item ranges [a, b) covering every item in order, each of at most `limit` listed devices (an item
    longer than `limit` gets a chunk of its own): a call's items are split at item boundaries only."""
    out: List[Tuple[int, int]] = []
    if len(lens) and int(np.sum(lens)) <= limit:  # the usual call: one chunk, no walk over the items
        return [(0, len(lens))]
    a, tot = 0, 0
    for i, n in enumerate(lens):
        n = int(n)
        if i > a and tot + n > limit:
            out.append((a, i))
            a, tot = i, 0
        tot += n
    if len(lens) > a:
        out.append((a, len(lens)))
    return out


def gather_table(table: FleetTable, parent: np.ndarray, sub_off: np.ndarray, sub_idx: np.ndarray) -> FleetTable:
    """The FleetTable of the items' materialised lists -- item i = fleet i, its devices the listed ones in
    list order -- gathered with NumPy from the packed parent `table`: array for array what fleet_table
    makes of `[[fleets[f][j] for j in s] for f, s in items]`, the packer's blocks and kappa heads (first
    listed is_head device, else the first listed) included, so fleet_constants and the result builder run
    on it unchanged. Raises the packer's ZeroDivisionError where a list's own head makes it arise."""
    lens = np.diff(sub_off)
    g = np.repeat(table.dev_off[np.asarray(parent, np.int64)], lens) + sub_idx
    blocks = getattr(table, "_blocks", None)
    if blocks is not None:
        _, u8, f64, b64 = blocks
    else:
        u8 = np.stack([table.os_class, table.flags])
        f64 = np.stack([getattr(table, f) for f in F64_FIELDS])
        b64 = np.stack([getattr(table, f) for f in BYTE_FIELDS])
    # np.take along the device axis (the indices are validated: no per-element range check), several times
    # faster than a[:, g] on these blocks
    gu8, gf64, gb64 = (np.take(a, g, axis=1, mode="clip") for a in (u8, f64, b64))
    off = np.ascontiguousarray(sub_off, np.int64)
    tot = int(off[-1])
    at = np.where((gu8[1] & DEV_HEAD) != 0, np.arange(tot, dtype=np.int64), tot)
    first = np.minimum.reduceat(at, off[:-1]) if len(lens) else np.zeros(0, np.int64)
    heads = np.where(first < off[1:], first, off[:-1]).astype(np.int64)
    t = object.__new__(FleetTable)
    d = t.__dict__
    d["dev_off"], d["os_class"], d["flags"] = off, gu8[0], gu8[1]
    for j, f in enumerate(F64_FIELDS):
        d[f] = gf64[j]
    for j, f in enumerate(BYTE_FIELDS):
        d[f] = gb64[j]
    t.check(heads)
    d["_blocks"] = (off, gu8, gf64, gb64)
    d["_heads"] = heads
    return t


class ItemTable:
    """What halda.py's _batch_results and open_x_offsets read of a fleet table, for the items seen as fleets:
    dev_off (the items' sub_off), os_class (the listed devices' classes in list order), heads (kappa's head
    of each item, a device index of the parent table) and consts = (sum t_comm, sum xi, kappa) per item."""

    def __init__(self, dev_off, os_class, heads, consts):
        self.dev_off, self.os_class, self.heads, self.consts = dev_off, os_class, heads, consts

    @property
    def n_fleets(self) -> int:
        return int(self.dev_off.shape[0] - 1)

    def sizes(self) -> np.ndarray:
        return np.diff(self.dev_off)


def item_table(table: FleetTable, parent: np.ndarray, sub_off: np.ndarray, sub_idx: np.ndarray,
               model: ModelProfile) -> ItemTable:
    """The ItemTable of validated items: by the C packer's consts_items straight from the packed parent table
    and the index arrays -- the same scalar loops as its consts on the materialised fleets, so the same
    bits, with nothing of the size of the listed devices built but their class bytes -- else (no C packer,
    or a table without its blocks) from gather_table. Raises the packer's ZeroDivisionError where a list's
    own head has s_disk 0."""
    blocks = getattr(table, "_blocks", None)
    off = np.ascontiguousarray(sub_off, np.int64)
    if _PACKER is None or blocks is None or not hasattr(_PACKER, "consts_items"):
        gt = gather_table(table, parent, off, sub_idx)
        g = np.repeat(table.dev_off[np.asarray(parent, np.int64)], np.diff(off)) + sub_idx
        return ItemTable(off, gt.os_class, g[gt._heads], fleet_constants(gt, model))
    toff, u8, f64, b64 = blocks
    n = len(parent)
    out, cls, heads = np.empty((3, n)), np.empty(int(off[-1]), np.uint8), np.empty(n, np.int64)
    fout = "b_1" in model.f_out
    _PACKER.consts_items(f64, b64, u8, toff, np.ascontiguousarray(parent, np.int32), off,
                         np.ascontiguousarray(sub_idx, np.int32), fout, float(model.f_out["b_1"]) if fout else 0.0,
                         float(model.b_in), float(model.b_out), float(model.V), out, cls, heads)
    if np.any(table.s_disk[heads] == 0.0):  # FleetTable.check's head rule; its other rules held for the parents
        raise ZeroDivisionError("float division by zero")
    return ItemTable(off, cls, heads, (out[0], out[1], out[2]))


def check_item_heads(fleets, table: FleetTable, parent: np.ndarray, heads: np.ndarray, model: ModelProfile) -> None:
    """The packer's ValueError that depends on which device is kappa's head: with "b_1" in f_out but not in
    f_q, a CPU FLOPs row of the model's quantization without "b_1" is an error only on the head
    (fleet_table_py: `elif fq or (fout and i == head)`), so a parent packs while a list that makes such a
    device its head must raise as its materialised fleet would. The table cannot tell that row from an
    absent one (neither sets DEV_CPU_RATE), so the few heads without the flag are looked up in `fleets`."""
    if "b_1" not in model.f_out or "b_1" in model.f_q:
        return  # with f_q every such row raised when its parent was packed; without f_out nothing reads it
    for i in np.flatnonzero((table.flags[heads] & DEV_CPU_RATE) == 0).tolist():
        f = int(parent[i])
        sc = fleets[f][int(heads[i] - table.dev_off[f])].scpu
        row = sc.get(model.Q) if sc else None
        if row is not None and "b_1" not in row:
            raise ValueError(f"Batch size 1 (key 'b_1') not found in S_by_q[{model.Q}]")


def solve_items(table: FleetTable, parent: np.ndarray, sub_off: np.ndarray, sub_idx: np.ndarray,
                model: ModelProfile, pos: List[int], kv_factor: float, device: int = 0, fleets=None
                ) -> List[Optional[HALDAResult]]:
    """One halda_solve_subfleets_host call: the parent table and the item arrays go to the GPU, the items'
    x / c of the k that can be optimal come back (open_x_offsets over the list lengths), and halda.py's
    _batch_results builds each HALDAResult from them and the items' constants and classes (item_table)."""
    gt = item_table(table, parent, sub_off, sub_idx, model)
    if fleets is not None:
        check_item_heads(fleets, table, parent, gt.heads, model)
    ctx = get_context(device)  # (after the items' own errors: those need no GPU)
    n, tot, nk = len(parent), int(sub_off[-1]), len(pos)
    lens = np.diff(sub_off)
    xsel = open_x_offsets(gt, model, pos)
    ext = int(np.max(xsel + np.repeat(7 * lens + 1, nk), initial=0)) if (xsel >= 0).any() else 0
    fbuf, ibuf = _scratch("subsolve", ((n + n * nk + 2 * ext, np.float64), (n + 2 * tot + n * nk, np.int32)),
                          pinned=True)
    (xs_pin,) = _scratch("subxoff", (((len(xsel),), np.int64),), pinned=True)
    xs_pin[:] = xsel
    pf, pi = fbuf.ctypes.data, ibuf.ctypes.data
    o1, o2 = n, n + n * nk
    res = FleetSolve(best_k=ibuf[:n], obj_value=fbuf[:n], w=ibuf[n:n + tot], n=ibuf[n + tot:n + 2 * tot],
                     obj_by_k=fbuf[o1:o2].reshape(n, nk), status=ibuf[n + 2 * tot:].reshape(n, nk), ks=pos,
                     x=fbuf[o2:o2 + ext], c=fbuf[o2 + ext:], x_off=xs_pin)
    r = HaldaFleetResultC(pi, pf, pi + 4 * n, pi + 4 * (n + tot), pf + 8 * o1, pi + 4 * (n + 2 * tot), pf + 8 * o2,
                          pf + 8 * (o2 + ext), xs_pin.ctypes.data)
    fs, keep = _host_struct(table)
    # the item arrays in page-locked memory too, like the table and the results: every copy of the call a DMA
    pp, po, px = _scratch("subitems", (((n,), np.int32), ((n + 1,), np.int64), ((max(tot, 1),), np.int32)), pinned=True)
    pp[:], po[:], px[:tot] = parent, sub_off, sub_idx
    parent, sub_off, sub_idx = pp, po, px
    it = HaldaSubfleetsC(n, int(lens.min()), int(lens.max()), ptr(parent), ptr(sub_off), ptr(sub_idx))
    karr = np.asarray(pos, np.int32)
    m = model_struct(model, kv_factor)
    ctx.call("halda_solve_subfleets_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
             karr.ctypes.data, nk, ctypes.byref(r))
    del keep
    return _batch_results(gt, res, pos, model, consts=gt.consts)


def _solve_arrays(fleets, model, parent, sub_off, sub_idx, k_candidates, kv_bits, device):
    """The items (validated arrays) over `fleets`, chunk by chunk: each parent packed once."""
    Ks = _batch_k_list(model, k_candidates)  # halda_solve_batch's k list and k rules
    kv_factor = kv_bits_to_factor(kv_bits)
    n = len(parent)
    if n == 0:
        return []
    pos = _positive_ks(Ks)
    table = fleet_table(fleets, model, _reuse=True)
    if not pos:
        return [None] * n
    chunks = plan_chunks(np.diff(sub_off), SUBFLEET_CHUNK_DEVICES)
    if len(chunks) == 1:  # the usual call: the result builder's list as it is
        return solve_items(table, parent, sub_off, sub_idx, model, pos, kv_factor, device, fleets)
    out: List[Optional[HALDAResult]] = []
    for a, b in chunks:
        lo, hi = int(sub_off[a]), int(sub_off[b])
        out.extend(solve_items(table, parent[a:b], sub_off[a:b + 1] - lo, sub_idx[lo:hi], model, pos, kv_factor,
                               device, fleets))
    return out


def halda_solve_subfleets(
    fleets: Sequence[Sequence[DeviceProfile]],
    model: ModelProfile,
    items: Sequence[Tuple[int, Sequence[int]]],
    k_candidates: Optional[Iterable[int]] = None,
    mip_gap: Optional[float] = 1e-4,
    kv_bits: str = "8bit",
    device: int = 0,
) -> List[Optional[HALDAResult]]:
    """`halda_solve_batch([[fleets[f][j] for j in s] for f, s in items], ...)` without materialising the
    lists: result[i] is exactly that call's entry i (w, n and sets indexed within the list, the same
    obj_value bits, None where no k is feasible). Indices are local to fleet f, in any order, repeats
    allowed. IndexError for an index out of range, ValueError for an empty list."""
    fleets = fleets if isinstance(fleets, (list, tuple)) else list(fleets)
    sizes = np.asarray([len(d) for d in fleets], np.int64)
    parent, sub_off, sub_idx = pack_items(sizes, list(items))
    return _solve_arrays(fleets, model, parent, sub_off, sub_idx, k_candidates, kv_bits, device)


def leave_one_out_items(sizes: Sequence[int]):
    """(parent, sub_off, sub_idx) of every leave-one-out list of fleets of `sizes` devices, fleet by fleet,
    entry i of a fleet being the fleet without device i; a one-device fleet has no item (its only list
    would be empty)."""
    sizes = np.asarray(sizes, np.int64)
    counts = np.where(sizes >= 2, sizes, 0)
    tmpl = {}
    for M in np.unique(sizes[sizes >= 2]).tolist():
        j = np.arange(M - 1, dtype=np.int32)[None, :]
        tmpl[M] = (j + (j >= np.arange(M, dtype=np.int32)[:, None])).ravel()  # row i: 0 .. M - 1 without i
    parts = [tmpl[M] for M in sizes.tolist() if M >= 2]
    sub_idx = np.concatenate(parts) if parts else np.zeros(0, np.int32)
    parent = np.repeat(np.arange(len(sizes), dtype=np.int32), counts)
    sub_off = np.zeros(len(parent) + 1, np.int64)
    np.cumsum(np.repeat(sizes - 1, counts), out=sub_off[1:])
    return parent, sub_off, sub_idx


def halda_leave_one_out_batch(
    fleets: Sequence[Sequence[DeviceProfile]],
    model: ModelProfile,
    k_candidates: Optional[Iterable[int]] = None,
    mip_gap: Optional[float] = 1e-4,
    kv_bits: str = "8bit",
    device: int = 0,
) -> List[List[Optional[HALDAResult]]]:
    """Per fleet, the list whose entry i is `halda_solve_batch` of the fleet without device i (None where
    no k is feasible; [None] for a one-device fleet), all fleets' lists in one GPU call per chunk of
    SUBFLEET_CHUNK_DEVICES listed devices."""
    fleets = fleets if isinstance(fleets, (list, tuple)) else list(fleets)
    sizes = [len(d) for d in fleets]
    parent, sub_off, sub_idx = leave_one_out_items(sizes)
    # The output lists are made BEFORE the solve and filled by index afterwards: the result builder makes its
    # ~9 containers per result with the cyclic GC paused (fleetpack.c results), so the first container
    # allocated after it would start a collection that walks all of them (several ms per 4,096 results).
    # halda_solve_batch returns the builder's list as it is; this entry allocates nothing after it either.
    n_f = len(sizes)
    out = [[None] * M for M in sizes]
    flat = _solve_arrays(fleets, model, parent, sub_off, sub_idx, k_candidates, kv_bits, device)
    a = 0
    for f in range(n_f):
        M = sizes[f]
        if M >= 2:
            o = out[f]
            for i in range(M):
                o[i] = flat[a + i]
            a += M
    return out


def halda_leave_one_out(
    devs: Sequence[DeviceProfile],
    model: ModelProfile,
    k_candidates: Optional[Iterable[int]] = None,
    mip_gap: Optional[float] = 1e-4,
    kv_bits: str = "8bit",
    device: int = 0,
) -> List[Optional[HALDAResult]]:
    """The plan if device i drops out, for every i: entry i is `halda_solve_batch` of the fleet without
    device i (None where no k is feasible). A one-device fleet gives [None]."""
    return halda_leave_one_out_batch([list(devs)], model, k_candidates, mip_gap, kv_bits, device)[0]


def halda_select_devices(
    devs: Sequence[DeviceProfile],
    model: ModelProfile,
    k_candidates: Optional[Iterable[int]] = None,
    mip_gap: Optional[float] = 1e-4,
    kv_bits: str = "8bit",
    device: int = 0,
    _solve_lists: Optional[Callable[[List[List[int]]], List[Optional[HALDAResult]]]] = None,
) -> Tuple[List[int], HALDAResult]:
    """Which devices to leave out: greedy backward elimination on top of leave-one-out. Starting from the
    full fleet, each round solves the kept devices without each one of them and drops the device whose
    removal gives the lowest obj_value strictly below the current one (ties: the lowest index); it stops
    when no removal improves or one device is left. Returns (kept indices into `devs`, ascending; the
    HALDAResult of that sub-fleet, indexed within the kept list). A heuristic over subsets (at most
    M (M + 1) / 2 of them), not the optimum over all 2^M. RuntimeError when neither the fleet nor any
    sub-fleet met on the way is feasible. `_solve_lists` (tests): the solve of a list of index lists."""
    devs = list(devs)
    if not devs:
        raise IndexError("list index out of range")  # the reference's kappa on an empty fleet

    def on_gpu(lists):
        return halda_solve_subfleets([devs], model, [(0, s) for s in lists], k_candidates, mip_gap, kv_bits, device)

    solve = _solve_lists or on_gpu
    kept = list(range(len(devs)))
    cur = solve([kept])[0]
    while len(kept) > 1:
        res = solve([kept[:i] + kept[i + 1:] for i in range(len(kept))])
        best, best_obj = -1, cur.obj_value if cur is not None else float("inf")
        for i, r in enumerate(res):
            if r is not None and r.obj_value < best_obj:  # strict: ties stay with the lowest index
                best, best_obj = i, r.obj_value
        if best < 0:
            break
        cur = res[best]
        del kept[best]
    if cur is None:
        raise RuntimeError("No feasible MILP found for any k this round.")
    return kept, cur
