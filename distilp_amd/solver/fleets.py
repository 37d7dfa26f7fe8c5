"""Whole k-sweeps on the GPU from a flat device-field table (libhalda `halda_solve_fleets`).

`halda_solve` (halda.py) runs one fleet through this path and forms obj_value from
the returned c and x with NumPy, exactly as the reference forms it;
`halda_solve_fleets` below is the throughput / streaming entry on the same
kernels (obj_value formed on the GPU). Fleets are packed into a
`FleetTable` (one entry per device, the fields the reference's formulas read,
dense_common.py:25-230), and libhalda's fused sweep builds every (fleet, k) MILP's
per-device records in registers from the table (the records decoding the lowered
CSR would give; no MILP is materialised), solves it exactly and keeps the best k by
the reference's rule (ascending k, strict "<", halda_p_solver.py:407); the CSR
pipeline (GPU lowering bit-identical to `lower.lower_fleet`, then the milp()
replacement kernels) stays behind `set_fleets_path("csr")`. Only the
table goes over PCIe (~1.9 KB per 64-device fleet instead of ~160 KB of lowered
MILPs), and re-profiled fleets (config C5) never touch per-device Python
objects: `FleetTable.perturbed` rescales the table directly.

obj_value here is c.x + sum t_comm + sum xi + kappa formed on the GPU with c.x
summed in a fixed tree order: within 1e-12 relative of NumPy's dot (the host
path's). The table builder raises the reference's exceptions (ValueError for a
FLOPs table without batch key b_1, ZeroDivisionError for T_cpu == 0 or a zero
s_disk the objective constant divides by).
"""

from __future__ import annotations

import ctypes
import threading
from dataclasses import dataclass, replace
from typing import Iterable, List, Optional, Sequence

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._abi import (BYTE_FIELDS, F64_FIELDS, HaldaBatchC, HaldaBoundsC, HaldaBoxC, HaldaBudgetC,  # noqa: F401
                   HaldaChangeC, HaldaChangeFrontierC, HaldaFleetResultC, HaldaFleetsC, HaldaFrontierC, HaldaModelC,
                   HaldaPlanResultC, HaldaPlansC, HaldaResultC, HaldaSubfleetsC)  # (this module's names of old too)
from ._libhalda import HaldaUnavailable, failure, get_context, load_library, ptr
from .coefficients import HALDAResult, assign_sets, b_prime, gpu_flops_table, gpu_load_throughput
from .lower import kv_bits_to_factor

DEV_HEAD, DEV_UMA, DEV_CPU_RATE, DEV_GPU, DEV_GPU_RATE, DEV_CUDA_OK, DEV_METAL_OK, DEV_METAL_AVAIL = (
    1, 2, 4, 8, 16, 32, 64, 128)


def _bind(lib):
    """Kept for callers from before load_library declared every prototype itself: the library as it is."""
    return lib


_bind_plans = _bind_bounds = _bind_budget = _bind  # (the per-family names such callers know)


_MODEL_STRUCTS: dict = {}
_ABSENT = object()


def model_struct(model: ModelProfile, kv_factor: float) -> HaldaModelC:
    """The C ABI's halda_model of `model` at `kv_factor` (read-only for every caller). Remembered by the
    values it is made from -- every field it reads -- so a repeated halda_solve reuses it (a model
    edited between calls gives another key)."""
    fq, fo = model.f_q, model.f_out
    has_q, has_o = "b_1" in fq, "b_1" in fo
    key = (fq.get("b_1", _ABSENT), fo.get("b_1", _ABSENT), kv_factor, model.hk, model.ek, model.hv, model.ev,
           model.n_kv, model.b_layer, model.b_in, model.b_out, model.V, model.L)
    try:
        # (a zero anywhere: made afresh -- 0.0 and -0.0 are one dict key but not one struct)
        hit = None if 0.0 in key else _MODEL_STRUCTS.get(key)
    except TypeError:  # an unhashable field value: made afresh
        key, hit = None, None
    if hit is not None:
        return hit
    m = HaldaModelC(float(fq["b_1"]) if has_q else 0.0, float(fo["b_1"]) if has_o else 0.0, int(has_q),
                    int(has_o), float(b_prime(model, kv_bits_k=kv_factor)), float(model.b_layer),
                    float(model.b_in), float(model.b_out), float(model.V), int(model.L))
    if key is not None and 0.0 not in key:
        if len(_MODEL_STRUCTS) >= 64:
            _MODEL_STRUCTS.clear()
        _MODEL_STRUCTS[key] = m
    return m


@dataclass
class FleetTable:
    """Device fields of many fleets, one entry per device (fleet f = devices dev_off[f] .. dev_off[f+1]-1)."""

    dev_off: np.ndarray  # int64 [n_fleets + 1]
    os_class: np.ndarray  # uint8: 1 M1, 2 M2, 3 M3
    flags: np.ndarray  # uint8 DEV_*
    scpu_b1: np.ndarray
    sgpu_b1: np.ndarray
    T_cpu: np.ndarray
    T_gpu: np.ndarray
    t_kvcpy_cpu: np.ndarray
    t_kvcpy_gpu: np.ndarray
    t_ram2vram: np.ndarray
    t_vram2ram: np.ndarray
    t_comm: np.ndarray
    s_disk: np.ndarray
    d_avail_ram: np.ndarray  # float64 (integer byte counts, BYTE_FIELDS)
    c_cpu: np.ndarray
    c_gpu: np.ndarray
    d_avail_cuda: np.ndarray
    d_avail_metal: np.ndarray
    swap: np.ndarray

    @property
    def n_fleets(self) -> int:
        return int(self.dev_off.shape[0] - 1)

    @property
    def n_devices(self) -> int:
        return int(self.dev_off[-1])

    def sizes(self) -> np.ndarray:
        return np.diff(self.dev_off)

    def __setattr__(self, name, value):
        # a packed table's fields are rows of its _blocks, which _host_struct hands to libhalda
        # directly: reassigning a field detaches it, so the blocks no longer describe the table
        if name not in ("_blocks", "_heads") and "_blocks" in self.__dict__:
            del self.__dict__["_blocks"]
            self.__dict__.pop("_heads", None)
        object.__setattr__(self, name, value)

    def sets(self, f: int):
        """{"M1", "M2", "M3"} index lists of fleet f (dense_common.py:149-167)."""
        cls = self.os_class[self.dev_off[f]:self.dev_off[f + 1]]
        return {f"M{s}": [int(i) for i in np.nonzero(cls == s)[0]] for s in (1, 2, 3)}

    def perturbed(self, rng: np.random.Generator, lo: float = 0.9, hi: float = 1.1) -> "FleetTable":
        """Every numeric field times an independent log-uniform factor in [lo, hi] (config C5: a
        re-profiled fleet); byte counts stay integers (floor). Flags and device classes are kept."""
        n = self.n_devices

        def lu():
            return np.exp(rng.uniform(np.log(lo), np.log(hi), n))

        upd = {f: getattr(self, f) * lu() for f in F64_FIELDS}
        upd.update({f: np.floor(getattr(self, f) * lu()) for f in BYTE_FIELDS})  # still integers
        return replace(self, **upd)

    def check(self, heads: Optional[np.ndarray] = None) -> None:
        """The reference's ZeroDivisionErrors (alpha: bp / T_cpu; kappa: head and M1/M3 s_disk).
        heads: global index of each fleet's kappa head (first is_head device, else its first)."""
        if np.any(self.T_cpu == 0.0):
            raise ZeroDivisionError("float division by zero")
        if heads is None:
            heads = np.empty(self.n_fleets, np.int64)
            for f in range(self.n_fleets):
                a, b = self.dev_off[f], self.dev_off[f + 1]
                hs = np.nonzero(self.flags[a:b] & DEV_HEAD)[0]
                heads[f] = a + (int(hs[0]) if len(hs) else 0)
        if np.any(self.s_disk[heads] == 0.0) or np.any((self.os_class != 2) & (self.s_disk == 0.0)):
            raise ZeroDivisionError("float division by zero")


def _rate(table, q, f_has_b1: bool, raise_on_missing: bool) -> tuple:
    """(present, value) of _sum_f_over_S's S[q]["b_1"] (dense_common.py:49-75): present when q is in
    the table with a "b_1" entry. The reference raises ValueError when "b_1" is in f and q is in S
    but S[q] lacks "b_1" (:62-64); with f lacking "b_1" the term is silently 0."""
    if table is None or q not in table:
        return False, 0.0
    row = table[q]
    if "b_1" not in row:
        if f_has_b1 and raise_on_missing:
            raise ValueError(f"Batch size 1 (key 'b_1') not found in S_by_q[{q}]")
        return False, 0.0
    return True, float(row["b_1"])


def _load_packer():
    """The C packer (distilp_amd/csrc/fleetpack.c, built in-tree next to this file by build())."""
    try:
        from . import _fleetpack
    except ImportError:
        return None
    return _fleetpack


_PACKER = _load_packer()


_TLS = threading.local()


class _HostBlock:
    """One block of page-locked host memory from libhalda (halda_host_alloc), freed with its last view.
    halda_solve_fleets_host DMAs straight from / to arrays that all lie in such blocks (include/halda.h)."""

    def __init__(self, nbytes: int):
        self.lib = load_library()
        p = ctypes.c_void_p()
        rc = self.lib.halda_host_alloc(nbytes, ctypes.byref(p))
        if rc != 0:
            raise failure(self.lib, f"halda_host_alloc({nbytes})", rc)
        self.ptr = p.value

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                self.lib.halda_host_free(self.ptr)
            except Exception:  # noqa: BLE001 -- interpreter teardown: the process's memory goes with it
                pass
            self.ptr = None


_PINNED_OK = True  # False once page-locked memory could not be had (no GPU runtime): pageable workspaces


def _host_arrays(shapes) -> tuple:
    """Arrays of `shapes` ((shape, dtype) each, 256-B aligned) carved from one _HostBlock."""
    offs, o = [], 0
    for sh, dt in shapes:
        offs.append(o)
        o += (int(np.prod(sh)) * np.dtype(dt).itemsize + 255) & ~255
    blk = _HostBlock(max(o, 256))
    raw = (ctypes.c_char * max(o, 256)).from_address(blk.ptr)
    raw._owner = blk  # the views keep the ctypes array alive, and it the block
    return tuple(np.frombuffer(raw, dt, int(np.prod(sh)), off).reshape(sh) for (sh, dt), off in zip(shapes, offs))


def _scratch(kind: str, shapes, pinned: bool = False) -> tuple:
    """The calling thread's reusable arrays for `kind` ((shape, dtype) each), kept between calls while the
    shapes repeat: a batch of 4,096 C3 fleets needs ~33 MB of table and ~30 MB of results, whose first
    touch of fresh pages costs more than the pass that fills them. One set per kind and thread. `pinned`:
    in page-locked memory (_host_arrays), so that the GPU call copies them by DMA with no staging copy."""
    ws = getattr(_TLS, "scratch", None)
    if ws is None:
        ws = _TLS.scratch = {}
    key = (pinned,) + tuple((tuple(np.atleast_1d(sh).tolist()), np.dtype(dt).str) for sh, dt in shapes)
    hit = ws.get(kind)
    if hit is None or hit[0] != key:
        global _PINNED_OK
        ws.pop(kind, None)  # the old set goes first (a pinned block is freed with its views)
        arrs = None
        if pinned and _PINNED_OK:
            try:
                arrs = _host_arrays(shapes)
            except (RuntimeError, OSError, ImportError):  # no GPU runtime here: pageable workspaces
                _PINNED_OK = False
        if arrs is None:
            arrs = tuple(np.empty(sh, dt) for sh, dt in shapes)
        hit = ws[kind] = (key, arrs)
    return hit[1]


def fleet_table(fleets: Sequence[Sequence[DeviceProfile]], model: ModelProfile, _reuse: bool = False) -> FleetTable:
    """Pack fleets (lists of DeviceProfile) into a FleetTable: one pass of the C packer over the
    devices into three field blocks (f64 [10][nd], int64 [6][nd], uint8 [2][nd]); the table's fields
    are rows of those blocks. Same values, flags and exceptions as fleet_table_py. `_reuse` (internal
    callers that are done with the table before their next call on this thread): the blocks are the
    thread's workspace, overwritten by the next such call."""
    if _PACKER is None:  # the C packer is not built for this interpreter: the Python packer (same table)
        return fleet_table_py(fleets, model)
    fleets = fleets if isinstance(fleets, (list, tuple)) else list(fleets)
    nf = len(fleets)
    nd = sum(len(d) for d in fleets)
    shapes = (((len(F64_FIELDS), nd), np.float64), ((len(BYTE_FIELDS), nd), np.float64), ((2, nd), np.uint8),
              (nf + 1, np.int64), (nf, np.int64))
    if _reuse:
        f64, b64, u8, off, heads = _scratch("table", shapes, pinned=True)
    else:
        f64, b64, u8, off, heads = (np.empty(sh, dt) for sh, dt in shapes)
    _PACKER.pack(fleets, model.Q, "b_1" in model.f_q, "b_1" in model.f_out, f64, b64, u8, off, heads)
    # the dataclass's fields set directly (no per-field __setattr__), then the packed blocks they view
    t = object.__new__(FleetTable)
    d = t.__dict__
    d["dev_off"], d["os_class"], d["flags"] = off, u8[0], u8[1]
    for j, f in enumerate(F64_FIELDS):
        d[f] = f64[j]
    for j, f in enumerate(BYTE_FIELDS):
        d[f] = b64[j]
    d["_blocks"] = (off, u8, f64, b64)  # FleetTable.check ran in the packer
    d["_heads"] = heads                  # kappa's head of each fleet (global device index)
    return t


def fleet_table_py(fleets: Sequence[Sequence[DeviceProfile]], model: ModelProfile) -> FleetTable:
    """The packer in Python (one row tuple per device, then one NumPy conversion per field group):
    the specification the C packer is tested against."""
    Q = model.Q
    fq, fout = "b_1" in model.f_q, "b_1" in model.f_out
    cls, flags, f64, i64, heads = [], [], [], [], []
    off = [0]
    os_code = {"mac_no_metal": 1, "mac_metal": 2}
    for devs in fleets:
        if not devs:
            raise IndexError("list index out of range")  # the reference's kappa on an empty fleet
        head = next((i for i, d in enumerate(devs) if d.is_head), 0)  # kappa's head (dense_common.py:214-219)
        heads.append(off[-1] + head)
        for i, d in enumerate(devs):
            g = d.__dict__  # pydantic v2 keeps field values here: plain dict reads, no descriptor per field
            os_type = g["os_type"]
            cls.append(os_code.get(os_type, 3))
            fl = (DEV_HEAD if g["is_head"] else 0) | (DEV_UMA if g["is_unified_mem"] else 0)
            # alpha reads scpu with f_q; kappa reads the head's scpu with f_out
            sc = g["scpu"]
            row = sc.get(Q) if sc else None
            v = 0.0
            if row is not None:
                if "b_1" in row:
                    v = float(row["b_1"])
                    fl |= DEV_CPU_RATE
                elif fq or (fout and i == head):
                    raise ValueError(f"Batch size 1 (key 'b_1') not found in S_by_q[{Q}]")
            has_metal, has_cuda = g["has_metal"], g["has_cuda"]
            # _gpu_table / _pick_T_gpu (dense_common.py:78-97): Metal preferred, truthiness tests
            table = g["sgpu_metal"] if has_metal and g["sgpu_metal"] else (
                g["sgpu_cuda"] if has_cuda and g["sgpu_cuda"] else None)
            tg = g["T_metal"] if has_metal and g["T_metal"] else (g["T_cuda"] if has_cuda and g["T_cuda"] else None)
            gv, tgv = 0.0, 1.0
            if table is not None and tg is not None:
                fl |= DEV_GPU
                gok, gv = _rate(table, Q, fq, True)
                if gok:
                    fl |= DEV_GPU_RATE
                tgv = float(tg)
            dc, dm = g["d_avail_cuda"], g["d_avail_metal"]
            if has_cuda and dc is not None:
                fl |= DEV_CUDA_OK
            if dm is not None:
                fl |= DEV_METAL_AVAIL | (DEV_METAL_OK if has_metal else 0)
            flags.append(fl)
            f64.append((v, gv, g["T_cpu"], tgv, g["t_kvcpy_cpu"], g["t_kvcpy_gpu"], g["t_ram2vram"], g["t_vram2ram"],
                        g["t_comm"], g["s_disk"]))
            i64.append((g["d_avail_ram"], g["c_cpu"], g["c_gpu"], dc or 0, dm or 0,
                        min(g["d_bytes_can_swap"], g["d_swap_avail"]) if os_type == "android" else 0))
        off.append(off[-1] + len(devs))
    fa = np.array(f64, dtype=np.float64).reshape(-1, len(F64_FIELDS))
    ia = np.array(i64, dtype=np.int64).reshape(-1, len(BYTE_FIELDS)).astype(np.float64)  # as the C packer
    t = FleetTable(dev_off=np.asarray(off, np.int64), os_class=np.asarray(cls, np.uint8),
                   flags=np.asarray(flags, np.uint8),
                   **{f: np.ascontiguousarray(fa[:, j]) for j, f in enumerate(F64_FIELDS)},
                   **{f: np.ascontiguousarray(ia[:, j]) for j, f in enumerate(BYTE_FIELDS)})
    t.check(np.asarray(heads, np.int64))
    return t


def _padded(table: "FleetTable", vals: np.ndarray, fill=0.0) -> np.ndarray:
    """[n_fleets, max_devices] view of a per-device array, fleet rows in device order, `fill` past a
    fleet's end (a reshape when every fleet has the same size)."""
    sizes = table.sizes()
    nf, mmax = table.n_fleets, int(sizes.max()) if table.n_fleets else 0
    if nf and int(sizes.min()) == mmax and int(table.dev_off[0]) == 0:
        return vals[:nf * mmax].reshape(nf, mmax)
    j = np.arange(mmax)
    idx = table.dev_off[:-1, None] + j[None, :]
    ok = j[None, :] < sizes[:, None]
    return np.where(ok, vals[np.where(ok, idx, 0)], fill)


def fleet_constants(table: "FleetTable", model: ModelProfile):
    """Per fleet (sum t_comm, sum xi, kappa): the constant part of obj_value in the reference's own
    order -- by the C packer's `consts` on a packed table (scalar loops, the bits of the reference's
    Python loops), else by fleet_constants_np."""
    blocks, heads = getattr(table, "_blocks", None), getattr(table, "_heads", None)
    if _PACKER is None or blocks is None or heads is None or not hasattr(_PACKER, "consts"):
        return fleet_constants_np(table, model)
    off, u8, f64, b64 = blocks
    out = np.empty((3, table.n_fleets))
    fout = "b_1" in model.f_out
    _PACKER.consts(f64, b64, u8, off, heads, fout, float(model.f_out["b_1"]) if fout else 0.0, float(model.b_in),
                   float(model.b_out), float(model.V), out)
    return out[0], out[1], out[2]


def fleet_constants_np(table: "FleetTable", model: ModelProfile):
    """Per fleet (sum t_comm, sum xi, kappa): the constant part of obj_value, each in the reference's
    own summation order (halda_p_solver.py:356-357: Python loops over the devices from 0; kappa
    dense_common.py:211-230: the head's four terms, then the M1 devices' and then the M3 devices'
    RAM-headroom terms in index order), as NumPy column sweeps over all fleets at once: every
    fleet's running sum takes the same additions in the same order as the scalar loop (padding adds
    +0.0, which leaves a sum that starts at +0.0 unchanged). The table's packer already raised the
    reference's errors (zero s_disk / T_cpu, a missing b_1)."""
    nf = table.n_fleets
    tc = _padded(table, table.t_comm)
    uma = (table.flags & DEV_UMA) != 0
    xi_dev = (table.t_ram2vram + table.t_vram2ram) * np.where(uma, 0.0, 1.0)
    xm = _padded(table, xi_dev)
    t_sum = np.zeros(nf)
    x_sum = np.zeros(nf)
    for i in range(tc.shape[1]):
        t_sum = t_sum + tc[:, i]
        x_sum = x_sum + xm[:, i]
    # kappa's head: the first is_head device of the fleet, else its first device
    head_local = np.argmax(_padded(table, (table.flags & DEV_HEAD).astype(np.int64), fill=0) != 0, axis=1)
    h = table.dev_off[:-1] + head_local
    scpu, Tc, sd, hflag = table.scpu_b1[h], table.T_cpu[h], table.s_disk[h], table.flags[h]
    has_fout = "b_1" in model.f_out
    f_out = float(model.f_out["b_1"]) if has_fout else 0.0
    rate = has_fout & ((hflag & DEV_CPU_RATE) != 0) & (scpu > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        total = np.where(rate, 0.0 + f_out / np.where(rate, scpu, 1.0), 0.0)
    bin_, bout, V = float(model.b_in), float(model.b_out), float(model.V)
    total = total + (bin_ / V + bout) / Tc
    total = total + bin_ / (V * sd)
    total = total + bout / sd
    # tail: M1 devices then M3 devices, each in index order
    cls = _padded(table, table.os_class.astype(np.int64), fill=0)
    rank = np.where(cls == 1, 0, np.where(cls == 3, 1, 2))
    order = np.argsort(rank * (cls.shape[1] + 1) + np.arange(cls.shape[1])[None, :], axis=1, kind="stable")
    term = ((table.c_cpu - table.d_avail_ram) - table.swap) / table.s_disk  # integer byte counts: exact
    tm = np.take_along_axis(np.where(rank < 2, _padded(table, term), 0.0), order, axis=1)
    tail = np.zeros(nf)
    for i in range(tm.shape[1]):
        tail = tail + tm[:, i]
    return t_sum, x_sum, total + tail


def open_x_offsets(table: "FleetTable", model: ModelProfile, ks: Sequence[int]) -> np.ndarray:
    """Compact x / c layout (halda_fleet_result.x_off) of the instances that can be optimal: W = L // k
    >= M_f (else sum lb(w) = M_f > W: infeasible) and W < 1e6; -1 elsewhere. [n_fleets * n_k]."""
    sizes = table.sizes()
    W = np.asarray([int(model.L) // int(k) for k in ks], np.int64)
    open_ = (W[None, :] >= sizes[:, None]) & (W[None, :] < 1_000_000)
    n = np.where(open_, 7 * sizes[:, None] + 1, 0).ravel()
    off = np.cumsum(n) - n
    return np.where(open_.ravel(), off, -1).astype(np.int64)


@dataclass
class FleetSolve:
    """Per fleet: best k (0 = none feasible), obj_value, w / n (device layout); per (fleet, k): obj, status."""

    best_k: np.ndarray
    obj_value: np.ndarray
    w: np.ndarray
    n: np.ndarray
    obj_by_k: np.ndarray  # [n_fleets, n_k]
    status: np.ndarray  # [n_fleets, n_k]
    ks: List[int]
    x: Optional[np.ndarray] = None  # [n_fleets, n_k, 7 max_devices + 1] when requested (want_x=True)
    c: Optional[np.ndarray] = None
    x_off: Optional[np.ndarray] = None  # want_x="open": [n_fleets * n_k] offsets into the flat x / c


def _fleets_struct(t: FleetTable, addr) -> HaldaFleetsC:
    s = HaldaFleetsC()
    s.n_fleets = t.n_fleets
    sz = t.sizes()
    s.min_devices, s.max_devices = int(sz.min()), int(sz.max())
    for f in ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS:
        setattr(s, f, addr(f))
    return s


def _host_struct(t: FleetTable) -> tuple:
    """(HaldaFleetsC on the table's host arrays, arrays to keep alive). A packed table's fields are
    rows of three blocks: four pointer reads instead of one per field."""
    blocks = getattr(t, "_blocks", None)
    if blocks is None:
        arrs = {f: np.ascontiguousarray(getattr(t, f)) for f in ("dev_off", "os_class", "flags") + F64_FIELDS
                + BYTE_FIELDS}
        return _fleets_struct(t, lambda f: arrs[f].ctypes.data), arrs
    off, u8, f64, b64 = blocks
    nd = u8.shape[1]
    s = HaldaFleetsC()
    s.n_fleets = t.n_fleets
    if t.n_fleets == 1:
        s.min_devices = s.max_devices = nd
    else:
        sz = np.diff(off)
        s.min_devices, s.max_devices = int(sz.min()), int(sz.max())
    s.dev_off = off.ctypes.data
    pu, pf, pi = u8.ctypes.data, f64.ctypes.data, b64.ctypes.data
    s.os_class, s.flags = pu, pu + nd
    for j, f in enumerate(F64_FIELDS):
        setattr(s, f, pf + 8 * nd * j)
    for j, f in enumerate(BYTE_FIELDS):
        setattr(s, f, pi + 8 * nd * j)
    return s, blocks


def _k_list(model: ModelProfile, k_candidates: Optional[Iterable[int]]) -> List[int]:
    if k_candidates:
        return sorted(set(int(k) for k in k_candidates))
    L = model.L
    return sorted({d for d in range(1, L) if L % d == 0}) if L > 1 else []


class MultiDeviceContext:
    """libhalda multi-device context (halda_init_multi): one context per GPU ordinal of one process;
    solve() deals a FleetTable's fleets out over them (halda_solve_fleets_multi)."""

    def __init__(self, devices: Sequence[int]):
        self.lib = load_library()
        self._lock = threading.Lock()  # the per-GPU contexts' staging buffers are not reentrant
        ords = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        self.ctx = ctypes.c_void_p()
        rc = self.lib.halda_init_multi(len(devices), ords, ctypes.byref(self.ctx))
        if rc != 0:
            raise failure(self.lib, f"halda_init_multi({list(devices)})", rc, HaldaUnavailable)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.halda_free_multi(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def solve(self, table: FleetTable, model: ModelProfile, ks: Sequence[int], kv_factor: float,
              want_x: bool = False) -> "FleetSolve":
        return solve_table(table, model, ks, kv_factor, want_x=want_x, _multi=self)


class _OneFleet:
    """Per-thread workspace of the single-fleet path (`solve_one`, i.e. every `halda_solve`): the
    packer's blocks, the C structs pointing at them and the result buffers for one (devices,
    k-candidates) shape, reused while the shape repeats -- no per-call allocation or struct filling.
    The results are overwritten by the thread's next call: callers copy what they keep."""

    def __init__(self, nd: int, ks: Sequence[int], L: int):
        nk = len(ks)
        self.nd, self.ks, self.L = nd, list(ks), L
        self.karr = np.asarray(self.ks, np.int32)
        self.f64 = np.empty((len(F64_FIELDS), nd))
        self.b64 = np.empty((len(BYTE_FIELDS), nd))
        self.u8 = np.empty((2, nd), np.uint8)
        self.off = np.empty(2, np.int64)
        self.heads = np.empty(1, np.int64)
        self.consts = np.empty(3)
        # halda_fleets: {int32 n_fleets, min_devices, max_devices; 19 pointers} = 21 u64 slots
        self.hdr = np.zeros(21, np.uint64)
        pu, pf, pi = self.u8.ctypes.data, self.f64.ctypes.data, self.b64.ctypes.data
        self.hdr[0] = 1 | (nd << 32)
        self.hdr[1] = nd
        self.hdr[2:5] = [self.off.ctypes.data, pu, pu + nd]
        self.hdr[5:15] = pf + 8 * nd * np.arange(len(F64_FIELDS), dtype=np.uint64)
        self.hdr[15:21] = pi + 8 * nd * np.arange(len(BYTE_FIELDS), dtype=np.uint64)
        self.fs = HaldaFleetsC.from_buffer(self.hdr)
        xs = 7 * nd + 1
        # x / c only of the k that can be optimal (L // k >= M: every device needs a layer), in the compact
        # layout of halda_fleet_result.x_off: xrow[j] = k_j's row of x / c, -1 for the others
        self.xrow = [-1] * nk
        n_open = 0
        for j, k in enumerate(self.ks):
            if L // k >= nd:
                self.xrow[j] = n_open
                n_open += 1
        self.x_off = np.asarray([r * xs if r >= 0 else -1 for r in self.xrow], np.int64)
        self.fbuf = np.zeros(1 + nk + 2 * max(n_open, 1) * xs)
        self.ibuf = np.zeros(1 + 2 * nd + nk, np.int32)
        pF, pI = self.fbuf.ctypes.data, self.ibuf.ctypes.data
        o2 = 1 + nk
        self.status = self.ibuf[1 + 2 * nd:]
        no = max(n_open, 1)
        self.x = self.fbuf[o2:o2 + no * xs].reshape(no, xs)
        self.c = self.fbuf[o2 + no * xs:].reshape(no, xs)
        self.res = HaldaFleetResultC(pI, pF, pI + 4, pI + 4 * (1 + nd), pF + 8, pI + 4 * (1 + 2 * nd), pF + 8 * o2,
                                     pF + 8 * (o2 + no * xs), self.x_off.ctypes.data)
        # the call's arguments made once (ndarray.ctypes and byref cost microseconds per call)
        self.karr_p, self.fs_ref, self.res_ref = self.karr.ctypes.data, ctypes.byref(self.fs), ctypes.byref(self.res)




def pack_one(devs: Sequence[DeviceProfile], model: ModelProfile, ks: Sequence[int]) -> "_OneFleet":
    """One fleet (the `halda_solve` path) packed by the C packer into the thread's workspace for the
    k-candidates `ks` (ascending, > 0); raises the reference's coefficient / kappa exceptions as
    fleet_table does. ws.u8[0] holds the device classes."""
    if _PACKER is None or not hasattr(_PACKER, "sets"):
        raise RuntimeError("pack_one needs the C packer (distilp_amd/csrc/fleetpack.c)")
    nd = len(devs)
    ws = getattr(_TLS, "one", None)
    if ws is None or ws.nd != nd or ws.ks != ks or ws.L != model.L:
        ws = _TLS.one = _OneFleet(nd, ks, model.L)
    _PACKER.pack([devs], model.Q, "b_1" in model.f_q, "b_1" in model.f_out, ws.f64, ws.b64, ws.u8, ws.off, ws.heads)
    return ws


def sweep_one(ws: "_OneFleet", model: ModelProfile, kv_factor: float, device: int = 0) -> "_OneFleet":
    """The packed fleet of `ws` swept over its k-candidates by halda_solve_fleets_host, x and c of the k
    that can be optimal returned (ws.status [n_k]; ws.x / ws.c [rows, 7 M + 1], k_j's row ws.xrow[j]),
    and its obj_value constants (sum t_comm,
    sum xi, kappa in the reference's order, the packer's C loops) in ws.consts. The thread's next call
    overwrites them."""
    ctx = get_context(device)
    m = model_struct(model, kv_factor)
    with ctx._lock:  # (every halda_solve's call: made directly, as the launches are, not through ctx.call)
        rc = ctx.lib.halda_solve_fleets_host(ctx.ctx, ctypes.byref(m), ws.fs_ref, ws.karr_p, len(ws.ks), ws.res_ref)
    if rc != 0:
        raise failure(ctx.lib, "halda_solve_fleets_host", rc)
    fo = model.f_out
    has_o = "b_1" in fo
    _PACKER.consts(ws.f64, ws.b64, ws.u8, ws.off, ws.heads, has_o, float(fo["b_1"]) if has_o else 0.0,
                   float(model.b_in), float(model.b_out), float(model.V), ws.consts)
    return ws


def solve_table(table: FleetTable, model: ModelProfile, ks: Sequence[int], kv_factor: float,
                device: int = 0, want_x: bool = False, _multi: Optional["MultiDeviceContext"] = None,
                _reuse: bool = False) -> FleetSolve:
    """halda_solve_fleets_host on a host FleetTable (synchronous). want_x: also x and the lowered c
    of every (fleet, k) (so the host can form obj_value exactly as the reference, with NumPy);
    want_x="open": only of the instances that can be optimal (open_x_offsets), flat, with x_off.
    `_reuse`: the result arrays are the thread's workspace (fleet_table), overwritten by the next such
    call; the library writes every entry of them."""
    ks = [int(k) for k in ks]
    if not ks:
        raise ValueError("no k-candidates")
    if ks[0] <= 0:
        raise ZeroDivisionError("integer division or modulo by zero")
    fs, keep = _host_struct(table)
    nf, nd, nk = table.n_fleets, table.n_devices, len(ks)
    # results in two buffers (f64, int32) viewed per field: two pointer reads
    xsel = open_x_offsets(table, model, ks) if want_x == "open" else None
    if xsel is not None:
        ext = int(np.max(xsel + np.repeat(7 * table.sizes() + 1, nk), initial=0)) if (xsel >= 0).any() else 0
        xs = 0
    else:
        xs = 7 * int(fs.max_devices) + 1 if want_x else 0
        ext = nf * nk * xs
    if _reuse:
        fbuf, ibuf = _scratch("solve", ((nf + nf * nk + 2 * ext, np.float64), (nf + 2 * nd + nf * nk, np.int32)),
                              pinned=True)
        if xsel is not None:  # x_off in page-locked memory too: every array of the call is, so it DMAs directly
            (xs_pin,) = _scratch("xoff", (((len(xsel),), np.int64),), pinned=True)
            xs_pin[:] = xsel
            xsel = xs_pin
    else:
        fbuf = np.zeros(nf + nf * nk + 2 * ext)
        ibuf = np.zeros(nf + 2 * nd + nf * nk, np.int32)
    pf, pi = fbuf.ctypes.data, ibuf.ctypes.data
    o1, o2 = nf, nf + nf * nk
    out = FleetSolve(best_k=ibuf[:nf], obj_value=fbuf[:nf], w=ibuf[nf:nf + nd], n=ibuf[nf + nd:nf + 2 * nd],
                     obj_by_k=fbuf[o1:o2].reshape(nf, nk), status=ibuf[nf + 2 * nd:].reshape(nf, nk), ks=ks)
    if xsel is not None:
        out.x, out.c, out.x_off = fbuf[o2:o2 + ext], fbuf[o2 + ext:], xsel
    elif want_x:
        out.x = fbuf[o2:o2 + ext].reshape(nf, nk, xs)
        out.c = fbuf[o2 + ext:].reshape(nf, nk, xs)
    r = HaldaFleetResultC(pi, pf, pi + 4 * nf, pi + 4 * (nf + nd), pf + 8 * o1, pi + 4 * (nf + 2 * nd),
                          pf + 8 * o2 if want_x else None, pf + 8 * (o2 + ext) if want_x else None,
                          xsel.ctypes.data if xsel is not None else None)
    karr = np.asarray(ks, np.int32)
    m = model_struct(model, kv_factor)
    args = (ctypes.byref(m), ctypes.byref(fs), karr.ctypes.data, nk, ctypes.byref(r))
    if _multi is None:
        ctx = get_context(device)
        ctx.call("halda_solve_fleets_host", ctx.ctx, *args)
        return out
    with _multi._lock:
        rc = _multi.lib.halda_solve_fleets_multi(_multi.ctx, *args)
    if rc != 0:
        raise failure(_multi.lib, "halda_solve_fleets_host", rc)  # (reported under the host entry's name)
    return out


def halda_solve_fleets(
    fleets: Sequence[List[DeviceProfile]],
    model: ModelProfile,
    k_candidates: Optional[Iterable[int]] = None,
    mip_gap: Optional[float] = 1e-4,
    kv_bits: str = "8bit",
    device: int = 0,
) -> List[Optional[HALDAResult]]:
    """Many `halda_solve` calls in one GPU k-sweep (lowering on the GPU). Returns one HALDAResult per
    fleet, or None where no k is feasible (where `halda_solve` would raise). Prints nothing."""
    kv_factor = kv_bits_to_factor(kv_bits)
    ks = _k_list(model, k_candidates)
    table = fleet_table(fleets, model)
    res = solve_table(table, model, ks, kv_factor, device)
    out: List[Optional[HALDAResult]] = []
    for f, devs in enumerate(fleets):
        if res.best_k[f] == 0:
            out.append(None)
            continue
        a, b = table.dev_off[f], table.dev_off[f + 1]
        out.append(HALDAResult(w=[int(v) for v in res.w[a:b]], n=[int(v) for v in res.n[a:b]], k=int(res.best_k[f]),
                               obj_value=float(res.obj_value[f]), sets=assign_sets(list(devs))))
    return out


def _check_counts(k, **counts) -> None:
    """set_budget's / set_change's integer arguments: each of `counts` a non-negative integer, k positive."""
    for name, v in counts.items():
        if isinstance(v, bool) or int(v) != v or v < 0:
            raise ValueError(f"{name}: {v!r} is not a non-negative integer")
    if int(k) < 1:
        raise ValueError(f"k = {k} must be positive")


class DeviceFleetTable:
    """A FleetTable resident in device memory (torch tensors) plus device result buffers, for
    back-to-back asynchronous halda_solve_fleets launches (bench / streaming): nothing crosses PCIe
    per launch except the k list (n_k int32, staged by the call)."""

    def __init__(self, table: FleetTable, model: ModelProfile, ks: Sequence[int], kv_factor: float, torch_device,
                 want_per_k: bool = False):
        import torch

        self.table = table
        self.ks = np.asarray([int(k) for k in ks], np.int32)
        self.arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(torch_device)
                     for f in ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS}
        nf, nd, nk = table.n_fleets, table.n_devices, len(self.ks)
        self.out = {"best_k": torch.empty(nf, dtype=torch.int32, device=torch_device),
                    "obj_value": torch.empty(nf, dtype=torch.float64, device=torch_device),
                    "w": torch.empty(nd, dtype=torch.int32, device=torch_device),
                    "n": torch.empty(nd, dtype=torch.int32, device=torch_device)}
        if want_per_k:
            self.out["obj_by_k"] = torch.empty(nf * nk, dtype=torch.float64, device=torch_device)
            self.out["status"] = torch.empty(nf * nk, dtype=torch.int32, device=torch_device)
        self.fs = _fleets_struct(table, lambda f: self.arrs[f].data_ptr())
        self.res = HaldaFleetResultC(*(ptr(self.out.get(f)) for f in ("best_k", "obj_value", "w", "n", "obj_by_k",
                                                                      "status")))
        self.model = model_struct(model, kv_factor)
        self._plans = {}
        self.epoch = 0  # bumped whenever the prepared plans are freed (PlanRotation re-reads the handles)

    def nbytes(self) -> int:
        return sum(int(t.numel() * t.element_size()) for t in self.arrs.values())

    def _sweep_args(self) -> tuple:
        """(model, fleets, ks, n_k, out): what every sweep entry takes between its context and its stream."""
        return (ctypes.byref(self.model), ctypes.byref(self.fs), self.ks.ctypes.data, len(self.ks),
                ctypes.byref(self.res))

    def _tensor(self, a, count: int, what: str, fill=None, dtype=None, cast=np.int32):
        """`a` -- a tensor, an array or None -- as an owned contiguous tensor of `count` entries of `dtype` (int32
        unless given) on the table's device. None gives a tensor of `fill`, or None where there is no fill.
        What is no tensor becomes a NumPy array of dtype `cast` first (None: of its own dtype). ValueError,
        naming the `what` array, for another count."""
        import torch

        dev, dtype = self.out["best_k"].device, dtype or torch.int32
        if a is None:
            return None if fill is None else torch.full((count,), fill, dtype=dtype, device=dev)
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, cast))
        if t.numel() != count:
            raise ValueError(f"{what} array of {t.numel()} entries, expected {count}")
        return t.to(device=dev, dtype=dtype).contiguous().clone()

    def plan(self, ctx):
        """The prepared launch of this table on `ctx` (halda_fleets_plan_create: kernel choice, grids and
        kernel arguments derived once), created on first use and kept with the table (a set_fleets_path
        on ctx re-plans it at its next launch)."""
        if getattr(ctx, "ctx", None) is None:
            raise RuntimeError("DeviceFleetTable.plan: the context is closed")
        p = self._plans.get(id(ctx))
        if p is not None and p[0] is not ctx:  # a new context at a recycled id()
            p = None
        if p is None:
            h = ctypes.c_void_p()
            ctx.call("halda_fleets_plan_create", ctx.ctx, *self._sweep_args(), ctypes.byref(h))
            p = (ctx, h, ctx.lib.halda_fleets_plan_launch)
            self._plans[id(ctx)] = p
        return p

    def replan(self) -> None:
        """Free the prepared launches (the next launch prepares a new one). A PlanRotation over this
        table takes the new handles at its next launch; a PlanGroup keeps its own copy."""
        for ctx, h, _ in self._plans.values():
            ctx.lib.halda_fleets_plan_free(h)
        self._plans.clear()
        self.epoch += 1

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.replan()
        except Exception:
            pass

    def launch(self, ctx, stream: int) -> None:
        """Enqueue one k-sweep of every fleet on `stream` (a hipStream_t as int) through the prepared
        plan: one ctypes call, one or two kernel enqueues."""
        p = self._plans.get(id(ctx))
        c, h, fn = p if p is not None and p[0] is ctx and ctx.ctx is not None else self.plan(ctx)
        with ctx._lock:
            rc = fn(h, stream)
        if rc != 0:
            raise failure(ctx.lib, "halda_fleets_plan_launch", rc)

    def launch_unplanned(self, ctx, stream: int) -> None:
        """The same k-sweep through halda_solve_fleets (shapes re-derived on every call)."""
        ctx.call("halda_solve_fleets", ctx.ctx, *self._sweep_args(), ctypes.c_void_p(stream))

    def set_plans(self, k=None, w=None, n=None) -> None:
        """Give the table its resident plan: device tensors plan_k [n_fleets], plan_w / plan_n [n_devices]
        (int32; zeros, "no plan", where not given) and the evaluation's result buffers plan_out -- buffers of
        their own, next to what the constructor allocated. A streaming caller rewrites plan_k / plan_w /
        plan_n in place between launches (e.g. copies out["best_k"] / ["w"] / ["n"] into them)."""
        import torch

        dev = self.out["best_k"].device
        nf, nd = self.table.n_fleets, self.table.n_devices
        self.plan_k, self.plan_w, self.plan_n = (self._tensor(a, c, "plan", 0) for a, c in ((k, nf), (w, nd), (n, nd)))
        self.plan_out = {"status": torch.empty(nf, dtype=torch.int32, device=dev),
                         "obj_value": torch.empty(nf, dtype=torch.float64, device=dev),
                         "cycle": torch.empty(nf, dtype=torch.float64, device=dev),
                         "bottleneck": torch.empty(nf, dtype=torch.int32, device=dev),
                         "reason": torch.empty(nf, dtype=torch.int32, device=dev)}
        o = self.plan_out
        self._plans_c = HaldaPlansC(ptr(self.plan_k), ptr(self.plan_w), ptr(self.plan_n))
        self._plan_res = HaldaPlanResultC(*(ptr(o[f]) for f in ("status", "obj_value", "cycle", "bottleneck",
                                                                "reason")))

    def launch_with_plans(self, ctx, stream: int) -> None:
        """Enqueue the k-sweep of every fleet and the evaluation of the resident plan on `stream`
        (halda_solve_fleets_plans): self.out as launch() leaves it, self.plan_out the incumbents' evaluation."""
        if getattr(self, "_plans_c", None) is None:
            self.set_plans()
        ctx.call("halda_solve_fleets_plans", ctx.ctx, *self._sweep_args()[:4], ctypes.byref(self._plans_c),
                 ctypes.byref(self._plan_res), ctypes.byref(self.res), ctypes.c_void_p(stream))

    def set_bounds(self, w_min=None, w_max=None, n_min=None, n_max=None) -> None:
        """Give the table its resident per-device layer bounds: device tensors bound_min / bound_max
        [n_devices] (int32; zeros / INT32_MAX, "no bound", where not given), buffers of their own. A streaming
        caller rewrites them in place between launches. With n_min or n_max given, bound_nmin / bound_nmax
        too (the n columns' box), and launch_with_bounds calls halda_solve_fleets_boxed."""
        nd = self.table.n_devices
        self.bound_min = self._tensor(w_min, nd, "bounds", 0)
        self.bound_max = self._tensor(w_max, nd, "bounds", 2**31 - 1)
        self._bounds_c = HaldaBoundsC(ptr(self.bound_min), ptr(self.bound_max))
        self.bound_nmin = self.bound_nmax = self._box_c = None
        if n_min is not None or n_max is not None:
            self.bound_nmin = self._tensor(n_min, nd, "bounds", 0)
            self.bound_nmax = self._tensor(n_max, nd, "bounds", 2**31 - 1)
            self._box_c = HaldaBoxC(ptr(self.bound_min), ptr(self.bound_max), ptr(self.bound_nmin),
                                    ptr(self.bound_nmax))

    def launch_with_bounds(self, ctx, stream: int) -> None:
        """Enqueue the k-sweep of every fleet within the resident bounds on `stream`
        (halda_solve_fleets_bounded; halda_solve_fleets_boxed when set_bounds got an n array): self.out as
        launch() leaves it."""
        if getattr(self, "_bounds_c", None) is None:
            self.set_bounds()
        name, bd = (("halda_solve_fleets_bounded", self._bounds_c) if self._box_c is None else
                    ("halda_solve_fleets_boxed", self._box_c))
        ctx.call(name, ctx.ctx, *self._sweep_args()[:4], ctypes.byref(bd), ctypes.byref(self.res),
                 ctypes.c_void_p(stream))

    def set_budget(self, k, w0, max_p: int, w_min=None, w_max=None) -> None:
        """Give the table its resident incumbents for halda_solve_fleets_budget: device tensors budget_w0
        [n_devices] (int32; the caller checks every w0_i >= 1 and every fleet's sum = L // k) and, where given,
        budget_min / budget_max, next to the frontier's result buffers budget_out: status / obj / moved
        [n_fleets, max_p + 1], w / n [max_p + 1, n_devices]. A streaming caller rewrites budget_w0 in place
        between launches (e.g. copies out["w"] into it). ValueError, as the other Python entries raise it, for
        a shape outside the launch's gate (budget.check_gate)."""
        import torch

        from .budget import check_gate  # (here: budget.py's own imports start from this module)

        sizes = self.table.sizes()
        _check_counts(k, max_p=max_p)
        check_gate(int(sizes.max()), int(sizes.min()), int(max_p), int(k))
        dev = self.out["best_k"].device
        nf, nd, P1 = self.table.n_fleets, self.table.n_devices, int(max_p) + 1

        if w0 is None:
            raise ValueError("set_budget needs the incumbents' w0")
        self.budget_k = int(k)
        self.budget_w0, self.budget_min, self.budget_max = (self._tensor(a, nd, "budget") for a in (w0, w_min, w_max))
        self.budget_out = {"status": torch.empty((nf, P1), dtype=torch.int32, device=dev),
                           "obj": torch.empty((nf, P1), dtype=torch.float64, device=dev),
                           "moved": torch.empty((nf, P1), dtype=torch.int32, device=dev),
                           "w": torch.empty((P1, nd), dtype=torch.int32, device=dev),
                           "n": torch.empty((P1, nd), dtype=torch.int32, device=dev)}
        o = self.budget_out
        self._budget_c = HaldaBudgetC(ptr(self.budget_w0), ptr(self.budget_min), ptr(self.budget_max), int(max_p))
        self._frontier_c = HaldaFrontierC(nd, *(ptr(o[f]) for f in ("status", "obj", "moved", "w", "n")))

    def launch_with_budget(self, ctx, stream: int) -> None:
        """Enqueue the move frontier of every fleet around the resident incumbents on `stream`
        (halda_solve_fleets_budget): self.budget_out. set_budget has checked the gate."""
        if getattr(self, "_budget_c", None) is None:
            raise RuntimeError("launch_with_budget: call set_budget first")
        ctx.call("halda_solve_fleets_budget", ctx.ctx, ctypes.byref(self.model), ctypes.byref(self.fs), self.budget_k,
                 ctypes.byref(self._budget_c), ctypes.byref(self._frontier_c), ctypes.c_void_p(stream))

    def set_change(self, k, items, w0, max_p: int, max_deficit: int, w_min=None, w_max=None) -> None:
        """Give the table its resident items and incumbents for halda_solve_change. `items` is (parent, sub_off,
        sub_idx) as subfleets.pack_items returns them (validated here against the table); w0 / w_min / w_max are
        laid out by sub_off (int32; the caller keeps every w0_i >= 0 and every item's deficit L // k - sum w0 in
        0 .. max_deficit -- the arrays given here are checked, later in-place rewrites are the caller's). Device
        tensors change_w0 / change_min / change_max and the result buffers change_out: status / obj / loaded /
        released [n_items, max_p + 1], w / n [max_p + 1, sub_off[-1]]. A streaming caller rewrites change_w0 in
        place between launches. ValueError for a shape outside the launch's gate (change.check_gate)."""
        import torch

        from .change import check_gate, check_w0  # (here: both modules' own imports start from this one)
        from .subfleets import check_items

        _check_counts(k, max_p=max_p, max_deficit=max_deficit)
        parent, sub_off, sub_idx = (np.ascontiguousarray(a, t) for a, t in zip(items, (np.int32, np.int64, np.int32)))
        check_items(self.table.sizes(), parent.astype(np.int64), sub_off, sub_idx.astype(np.int64))
        lens = np.diff(sub_off)
        if len(lens) == 0:
            raise ValueError("set_change needs at least one item")
        check_gate(int(lens.max()), int(lens.min()), int(max_p), int(max_deficit), int(k))
        if w0 is None:
            raise ValueError("set_change needs the items' w0")
        dev = self.out["best_k"].device
        n, tot, P1 = len(parent), int(sub_off[-1]), int(max_p) + 1
        if not torch.is_tensor(w0):
            check_w0(sub_off, np.asarray(w0), int(self.model.L) // int(k), int(max_deficit))
        self.change_k = int(k)
        # (as before the helper: these arrays reach torch in their own dtype and are cast there)
        self.change_items = (self._tensor(parent, n, "change", cast=None),
                             self._tensor(sub_off, n + 1, "change", dtype=torch.int64, cast=None),
                             self._tensor(sub_idx, tot, "change", cast=None))
        self.change_w0, self.change_min, self.change_max = (self._tensor(a, tot, "change", cast=None)
                                                            for a in (w0, w_min, w_max))
        self.change_out = {"status": torch.empty((n, P1), dtype=torch.int32, device=dev),
                           "obj": torch.empty((n, P1), dtype=torch.float64, device=dev),
                           "loaded": torch.empty((n, P1), dtype=torch.int32, device=dev),
                           "released": torch.empty((n, P1), dtype=torch.int32, device=dev),
                           "w": torch.empty((P1, tot), dtype=torch.int32, device=dev),
                           "n": torch.empty((P1, tot), dtype=torch.int32, device=dev)}
        o = self.change_out
        self._items_c = HaldaSubfleetsC(n, int(lens.min()), int(lens.max()), *(ptr(t) for t in self.change_items))
        self._change_c = HaldaChangeC(ptr(self.change_w0), ptr(self.change_min), ptr(self.change_max), int(max_p),
                                      int(max_deficit))
        self._change_frontier_c = HaldaChangeFrontierC(tot, *(ptr(o[f]) for f in
                                                              ("status", "obj", "loaded", "released", "w", "n")))

    def launch_with_change(self, ctx, stream: int) -> None:
        """Enqueue the change frontier of every resident item on `stream` (halda_solve_change): self.change_out.
        set_change has checked the gate."""
        if getattr(self, "_change_c", None) is None:
            raise RuntimeError("launch_with_change: call set_change first")
        ctx.call("halda_solve_change", ctx.ctx, ctypes.byref(self.model), ctypes.byref(self.fs),
                 ctypes.byref(self._items_c), self.change_k, ctypes.byref(self._change_c),
                 ctypes.byref(self._change_frontier_c), ctypes.c_void_p(stream))


class RcclComm:
    """An RCCL communicator owned by libhalda (halda_comm_init): one per rank, `world` ranks, the
    128-byte id from `RcclComm.unique_id()` on one rank handed to the others by any channel."""

    def __init__(self, world: int, rank: int, uid: bytes, device: int = 0):
        self.lib = load_library()
        self.comm = ctypes.c_void_p()
        rc = self.lib.halda_comm_init(ctypes.byref(self.comm), world, rank, uid, device)
        if rc != 0:
            raise failure(self.lib, "halda_comm_init", rc, HaldaUnavailable)

    @staticmethod
    def unique_id() -> bytes:
        lib = load_library()
        buf = ctypes.create_string_buffer(128)
        rc = lib.halda_comm_unique_id(buf)
        if rc != 0:
            raise failure(lib, "halda_comm_unique_id", rc)
        return buf.raw

    def close(self):
        if getattr(self, "comm", None):
            self.lib.halda_comm_destroy(self.comm)
            self.comm = None


class PlanRotation:
    """Prepared launches of several resident tables on one context, launched in rotation over
    streams by one C call per group of steps (halda_fleets_plan_launch_many): step i runs table
    i % len(tables) on stream i % len(streams). A streaming caller's loop without a Python round trip
    per batch."""

    def __init__(self, tables, ctx, streams):
        self.ctx = ctx
        self.lib = ctx.lib
        self.tables = list(tables)  # (the plans live with them)
        self.n_p, self.n_s = len(self.tables), len(streams)
        self.streams = (ctypes.c_void_p * self.n_s)(*[ctypes.c_void_p(int(x)).value for x in streams])
        self._take_plans()

    def _take_plans(self) -> None:
        self.plans = (ctypes.c_void_p * self.n_p)(*[t.plan(self.ctx)[1].value for t in self.tables])
        self.epochs = [t.epoch for t in self.tables]

    def launch(self, first: int, steps: int) -> None:
        if self.ctx.ctx is None:
            raise RuntimeError("PlanRotation.launch: the context is closed")
        if [t.epoch for t in self.tables] != self.epochs:  # a table re-planned: its old handle is freed
            self._take_plans()
        with self.ctx._lock:
            rc = self.lib.halda_fleets_plan_launch_many(self.plans, self.n_p, self.streams, self.n_s, first, steps)
        if rc != 0:
            raise failure(self.lib, "halda_fleets_plan_launch_many", rc)


class PlanGroup:
    """Resident tables run as a stream of batches by ONE launch (halda_fleets_group_launch): batch t of
    launch(first, steps, stream) is table (first + t) % len(tables), each batch's results in its own
    table's arrays, as PlanRotation over one stream would leave them. `persistent` tells whether the
    steps run as one launch (register sweeps of one shape: C3) or batch by batch."""

    def __init__(self, tables, ctx):
        self.ctx = ctx
        self.lib = ctx.lib
        self.tables = list(tables)  # the group reads their device arrays: they stay alive with it
        plans = (ctypes.c_void_p * len(self.tables))(*[t.plan(ctx)[1].value for t in self.tables])
        self.group = ctypes.c_void_p()
        pers = ctypes.c_int32(0)
        ctx.call("halda_fleets_group_create", plans, len(self.tables), ctypes.byref(self.group), ctypes.byref(pers))
        self.persistent = bool(pers.value)

    def launch(self, first: int, steps: int, stream: int) -> None:
        if self.ctx.ctx is None:
            raise RuntimeError("PlanGroup.launch: the context is closed")
        with self.ctx._lock:
            rc = self.lib.halda_fleets_group_launch(self.group, first, steps, ctypes.c_void_p(stream))
        if rc != 0:
            raise failure(self.lib, "halda_fleets_group_launch", rc)

    def close(self) -> None:
        if getattr(self, "group", None):
            self.lib.halda_fleets_group_free(self.group)
            self.group = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass


def launch_sharded_emulated(dt: "DeviceFleetTable", ctx, world: int, report_rank: int, stream: int) -> None:
    """Latency mode's step sequence for `world` virtual ranks on this one GPU
    (halda_solve_fleets_sharded_emulated): each RCCL all-reduce replaced, in order, by a device reduction
    over the virtual ranks' arrays; virtual rank `report_rank`'s results land in dt.out."""
    ctx.call("halda_solve_fleets_sharded_emulated", ctx.ctx, int(world), int(report_rank), *dt._sweep_args(),
             ctypes.c_void_p(stream))


def launch_sharded(dt: "DeviceFleetTable", ctx, comm: RcclComm, stream: int) -> None:
    """Latency mode over RCCL (halda_solve_fleets_sharded): this rank sweeps its share of dt's
    k-candidates and the ranks all-reduce to the same best k / obj_value / w / n (and obj_by_k / status
    when dt holds them) in dt.out, on every rank."""
    ctx.call("halda_solve_fleets_sharded", ctx.ctx, comm.comm, *dt._sweep_args(), ctypes.c_void_p(stream))
