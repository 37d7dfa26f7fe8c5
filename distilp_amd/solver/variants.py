"""One fleet table against many model variants (libhalda `halda_solve_variants`).

The question a planner asks before deploying is about the model: which KV precision and which context
length can this fleet serve, and at what cost? A variant is `(ModelProfile, kv_bits)`. The packed fleet
table reads only the model's quantization `Q` and whether `f_q` / `f_out` carry "b_1" (`fleet_table`), so
every variant that agrees on those and on `L` shares ONE table: it is packed once, uploaded once and solved
for all variants in one GPU call (one launch where the shape allows, else a loop of launches inside the
library). `out[v][f]` is exactly `halda_solve_batch(fleets, variants[v][0], ..., kv_bits=variants[v][1])[f]`:
the host constants (`fleet_constants`) and the objective (`_batch_results`) are formed per variant from that
variant's model, on that variant's slice of the returned x / c.
"""

from __future__ import annotations

import ctypes
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._abi import HaldaFleetResultC, HaldaModelC
from ._libhalda import get_context, last_route, set_path
from .coefficients import HALDAResult
from .fleets import FleetSolve, _host_struct, _scratch, fleet_constants, fleet_table, model_struct, open_x_offsets
from .fleets import _bind as _bind_var  # noqa: F401 -- the identity, for callers from before load_library bound all
from .halda import _batch_k_list, _batch_results, _positive_ks
from .lower import kv_bits_to_factor

Variant = Tuple[ModelProfile, str]

MAX_VARIANTS = 65535  # halda_solve_variants: blockIdx.y is the variant


def set_variants_path(ctx, path: int) -> None:
    """halda_set_variants_path on a HaldaContext: 0 automatic (default), 1 always loop (test path)."""
    set_path(ctx, "variants", path)


def last_variants_route(ctx) -> str:
    """The route of the context's last halda_solve_variants call: "fused", "loop" or "none"."""
    return last_route(ctx, "variants")


def model_grid(model: ModelProfile, kv_bits: Sequence[str] = ("8bit",), n_kv: Optional[Iterable[int]] = None
               ) -> List[Variant]:
    """The variants list of every (n_kv, kv_bits) pair, n_kv outermost: `model` with its n_kv replaced
    (n_kv=None: the model's own), at each KV precision."""
    kv_bits = [kv_bits] if isinstance(kv_bits, str) else list(kv_bits)
    ns = [int(model.n_kv)] if n_kv is None else [int(n) for n in n_kv]
    return [(model.model_copy(update={"n_kv": n}), kv) for n in ns for kv in kv_bits]


def check_variants(variants: Sequence[Variant]) -> None:
    """ValueError when the variants cannot share one packed table and one plan: they differ in L, in Q, or
    in whether "b_1" is in f_q / f_out."""
    if len(variants) > MAX_VARIANTS:
        raise ValueError(f"{len(variants)} variants: at most {MAX_VARIANTS} in one call")
    m0 = variants[0][0]
    for v, (m, _) in enumerate(variants):
        if int(m.L) != int(m0.L):
            raise ValueError(f"variant {v}: L = {m.L}, variant 0 has L = {m0.L}")
        if m.Q != m0.Q:
            raise ValueError(f"variant {v}: Q = {m.Q!r}, variant 0 has Q = {m0.Q!r}")
        if ("b_1" in m.f_q) != ("b_1" in m0.f_q):
            raise ValueError(f"variant {v} differs from variant 0 in whether 'b_1' is in f_q")
        if ("b_1" in m.f_out) != ("b_1" in m0.f_out):
            raise ValueError(f"variant {v} differs from variant 0 in whether 'b_1' is in f_out")


def variant_offsets(n_var: int, nf: int, nd: int, nk: int) -> dict:
    """Element offset of every variant's slice in each variant-major output of halda_solve_variants
    (include/halda.h): per output, an int64 array of n_var offsets."""
    v = np.arange(n_var, dtype=np.int64)
    return {"best_k": v * nf, "obj_value": v * nf, "w": v * nd, "n": v * nd, "obj_by_k": v * nf * nk,
            "status": v * nf * nk, "x_off": v * nf * nk}


def variant_x_offsets(xsel: np.ndarray, ext: int, n_var: int) -> np.ndarray:
    """The call's compact x / c layout: the per-table layout `xsel` (open_x_offsets: the same for every
    variant, it depends on L alone) repeated per variant, variant v's rows moved by v * ext elements; -1
    stays -1. [n_var * len(xsel)]."""
    base = (np.arange(n_var, dtype=np.int64) * int(ext))[:, None]
    return np.where(xsel[None, :] >= 0, xsel[None, :] + base, -1).astype(np.int64).ravel()


def model_structs(variants: Sequence[Variant]):
    """The C array of the variants' halda_model (model_struct of each)."""
    arr = (HaldaModelC * len(variants))()
    for v, (m, kv) in enumerate(variants):
        s = model_struct(m, kv_bits_to_factor(kv))
        ctypes.memmove(ctypes.byref(arr, v * ctypes.sizeof(HaldaModelC)), ctypes.byref(s), ctypes.sizeof(HaldaModelC))
    return arr


def variant_constants(table, variants: Sequence[Variant]) -> list:
    """Per variant the host constants (sum t_comm, sum xi, kappa) of every fleet: fleet_constants of the ONE
    packed table with that variant's model (kappa reads the variant's f_out["b_1"], b_in, b_out and V; the
    table's own fields do not depend on the variant)."""
    return [fleet_constants(table, m) for m, _ in variants]


def solve_variants_table(table, variants: Sequence[Variant], pos: List[int], device: int = 0) -> List[FleetSolve]:
    """One halda_solve_variants_host call on a packed table: per variant the FleetSolve (want_x="open") of
    its slice -- views of one result buffer, with the variant's x / c rows from 0 and the per-table x_off."""
    ctx = get_context(device)
    nv, nf, nd, nk = len(variants), table.n_fleets, table.n_devices, len(pos)
    m0 = variants[0][0]
    xsel = open_x_offsets(table, m0, pos)
    ext = int(np.max(xsel + np.repeat(7 * table.sizes() + 1, nk), initial=0)) if (xsel >= 0).any() else 0
    fbuf, ibuf = _scratch("varsolve", ((nv * (nf + nf * nk + 2 * ext), np.float64),
                                       (nv * (nf + 2 * nd + nf * nk), np.int32)), pinned=True)
    (xs_pin,) = _scratch("varxoff", (((nv * len(xsel),), np.int64),), pinned=True)
    xs_pin[:] = variant_x_offsets(xsel, ext, nv)
    pf, pi = fbuf.ctypes.data, ibuf.ctypes.data
    # f64: obj_value | obj_by_k | x | c; int32: best_k | w | n | status -- each variant-major
    f_obj, f_obk, f_x, f_c = 0, nv * nf, nv * (nf + nf * nk), nv * (nf + nf * nk + ext)
    i_bk, i_w, i_n, i_st = 0, nv * nf, nv * (nf + nd), nv * (nf + 2 * nd)
    r = HaldaFleetResultC(pi + 4 * i_bk, pf + 8 * f_obj, pi + 4 * i_w, pi + 4 * i_n, pf + 8 * f_obk, pi + 4 * i_st,
                          pf + 8 * f_x, pf + 8 * f_c, xs_pin.ctypes.data)
    fs, keep = _host_struct(table)
    karr = np.asarray(pos, np.int32)
    ms = model_structs(variants)
    ctx.call("halda_solve_variants_host", ctx.ctx, ms, nv, ctypes.byref(fs), karr.ctypes.data, nk, ctypes.byref(r))
    del keep
    o = variant_offsets(nv, nf, nd, nk)
    out = []
    for v in range(nv):
        a, d, q = int(o["best_k"][v]), int(o["w"][v]), int(o["status"][v])
        out.append(FleetSolve(best_k=ibuf[i_bk + a:i_bk + a + nf], obj_value=fbuf[f_obj + a:f_obj + a + nf],
                              w=ibuf[i_w + d:i_w + d + nd], n=ibuf[i_n + d:i_n + d + nd],
                              obj_by_k=fbuf[f_obk + q:f_obk + q + nf * nk].reshape(nf, nk),
                              status=ibuf[i_st + q:i_st + q + nf * nk].reshape(nf, nk), ks=pos,
                              x=fbuf[f_x + v * ext:f_x + (v + 1) * ext], c=fbuf[f_c + v * ext:f_c + (v + 1) * ext],
                              x_off=xsel))
    return out


def halda_solve_variants(
    fleets: Sequence[Sequence[DeviceProfile]],
    variants: Sequence[Variant],
    k_candidates: Optional[Iterable[int]] = None,
    mip_gap: Optional[float] = 1e-4,
    device: int = 0,
) -> List[List[Optional[HALDAResult]]]:
    """`[halda_solve_batch(fleets, m, k_candidates, mip_gap, kv) for m, kv in variants]` with the fleets
    packed once and all variants in one GPU call: out[v][f] is exactly that list's entry (the same k, w, n,
    sets and obj_value bits; None where no k is feasible). ValueError when the variants differ in L, in Q or
    in whether "b_1" is in f_q / f_out (the packed table would differ); [] for no variants."""
    variants = [(m, kv) for m, kv in variants]
    if not variants:
        return []
    check_variants(variants)
    m0 = variants[0][0]
    if k_candidates is not None and not isinstance(k_candidates, (list, tuple)):
        k_candidates = list(k_candidates)
    Ks = _batch_k_list(m0, k_candidates)  # halda_solve_batch's k list: it depends on L alone
    for _, kv in variants:
        kv_bits_to_factor(kv)  # an unknown precision raises before anything is packed
    fleets = fleets if isinstance(fleets, (list, tuple)) else list(fleets)
    if not Ks:
        return [[None] * len(fleets) for _ in variants]
    pos = _positive_ks(Ks)
    if not fleets:
        return [[] for _ in variants]
    table = fleet_table(fleets, m0, _reuse=True)
    if not pos:
        return [[None] * len(fleets) for _ in variants]
    consts = variant_constants(table, variants)
    solves = solve_variants_table(table, variants, pos, device)
    return [_batch_results(table, res, pos, m, consts=cs) for (m, _), res, cs in zip(variants, solves, consts)]


def halda_context_sweep(
    devs: Sequence[DeviceProfile],
    model: ModelProfile,
    n_kv: Optional[Iterable[int]] = None,
    kv_bits: Sequence[str] = ("4bit", "8bit", "fp16"),
    k_candidates: Optional[Iterable[int]] = None,
    mip_gap: Optional[float] = 1e-4,
    device: int = 0,
) -> List[Tuple[int, str, Optional[HALDAResult]]]:
    """One fleet over the (n_kv, kv_bits) grid of model_grid: rows (n_kv, kv_bits, HALDAResult or None where
    no k is feasible), n_kv outermost."""
    grid = model_grid(model, kv_bits, n_kv)
    res = halda_solve_variants([list(devs)], grid, k_candidates, mip_gap, device)
    return [(int(m.n_kv), kv, r[0]) for (m, kv), r in zip(grid, res)]
