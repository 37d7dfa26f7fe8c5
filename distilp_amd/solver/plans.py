"""A deployed plan priced on the fleet as it is now (libhalda `halda_eval_plans` / `halda_solve_fleets_plans`).

The k-sweep answers "what is the best plan for this fleet?". A re-placement decision needs the other half:
what does the plan that is running, `(k, w, n)`, cost on the re-profiled fleet, and is the new optimum
enough better to move layers? `halda_evaluate_plan` prices a fixed plan (the reference's answer for the
fixed-k MILP with the w / n columns fixed); `halda_replace_or_keep` sweeps and prices the incumbent in one
GPU call and reports the regret and the layers that would move.

`evaluate_plan_np` is the specification: the same reduction from the `FleetTable` arrays with NumPy, usable
without a GPU (the role `gather_table` has for sub-fleets).
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._abi import HaldaFleetResultC, HaldaPlanResultC, HaldaPlansC
from ._libhalda import (STATUS_INFEASIBLE, STATUS_OPTIMAL, STATUS_UNSUPPORTED, get_context, last_route, ptr,
                        set_path)
from .coefficients import HALDAResult, b_prime
from .fleets import (DEV_CPU_RATE, DEV_CUDA_OK, DEV_GPU, DEV_GPU_RATE, DEV_HEAD, DEV_METAL_AVAIL, DEV_METAL_OK,
                     DEV_UMA, FleetSolve, FleetTable, _host_struct, fleet_constants, fleet_table, model_struct,
                     open_x_offsets)
from .halda import _batch_k_list, _batch_results, _positive_ks
from .lower import kv_bits_to_factor

REASON_SUM_W, REASON_RANGE_W, REASON_RANGE_N, REASON_SLACK, REASON_RECORD, REASON_NO_PLAN = 1, 2, 4, 8, 16, 32
REASON_NAMES = ((REASON_SUM_W, "sum_w"), (REASON_RANGE_W, "w_out_of_range"), (REASON_RANGE_N, "n_out_of_range"),
                (REASON_SLACK, "slack_over_bound"), (REASON_RECORD, "record_rejected"), (REASON_NO_PLAN, "no_plan"))

SLACK_EPS = 1e-6  # csrc/halda_prims.hpp kSlackEps
_NO_ROW = -(1 << 29)  # csrc/halda_solve.hpp kNoRow

Plan = Tuple[int, Sequence[int], Sequence[int]]
Incumbent = Union[HALDAResult, Plan, None]


def set_plans_path(ctx, path: int) -> None:
    """halda_set_plans_path on a HaldaContext: 0 automatic (default: two launches), 1 always two launches,
    2 the fused launch where it applies."""
    set_path(ctx, "plans", path)


def last_plans_route(ctx) -> str:
    """The route of the context's last halda_solve_fleets_plans call: "fused", "two_launch" or "none"."""
    return last_route(ctx, "plans")


def reason_names(reason: int) -> Tuple[str, ...]:
    return tuple(name for bit, name in REASON_NAMES if reason & bit)


@dataclass(frozen=True)
class PlanEvaluation:
    """One plan priced on one fleet. obj_value / cycle_time are +inf and bottleneck None unless feasible."""

    feasible: bool
    obj_value: float
    cycle_time: float
    bottleneck: Optional[int]
    reasons: Tuple[str, ...] = ()
    status: int = STATUS_OPTIMAL
    reason: int = 0


@dataclass(frozen=True)
class Replacement:
    """halda_replace_or_keep's answer: the incumbent priced on the fleet, the new optimum (None where no k is
    feasible), regret = incumbent.obj_value - best.obj_value (inf for an infeasible incumbent),
    moved_layers = sum_i |w_i^best - w_i^incumbent| (0 without an incumbent or a best), and the verdict."""

    incumbent: PlanEvaluation
    best: Optional[HALDAResult]
    regret: float
    moved_layers: int
    replace: bool


# ------------------------------------------------------------------ the specification (NumPy, no GPU)
def _f_over_s(present, f, s):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = 0.0 + f / np.where(s > 0.0, s, 1.0)
    return np.where(present & (s > 0.0), q, 0.0)


def plan_records(table: FleetTable, model: ModelProfile, f: int, kv_factor: float) -> dict:
    """The device records of fleet f as the sweep's field_rec builds them (csrc/halda_sweep.hpp: dev_coef,
    rhs_*, the least-slack offsets K = ceil(-rhs / b' - eps)), in its operation order: arrays over the fleet's
    devices. `bad` marks a record field_rec rejects."""
    a, b_ = int(table.dev_off[f]), int(table.dev_off[f + 1])
    g = lambda name: np.asarray(getattr(table, name)[a:b_], np.float64)  # noqa: E731
    fl = np.asarray(table.flags[a:b_], np.int64)
    cls = np.asarray(table.os_class[a:b_], np.int64)
    bp = float(b_prime(model, kv_bits_k=kv_factor))
    has_fq = "b_1" in model.f_q
    fq = float(model.f_q["b_1"]) if has_fq else 0.0
    b_in, b_out, V, b_layer = float(model.b_in), float(model.b_out), float(model.V), float(model.b_layer)
    bvo = (b_in / V) + b_out
    Tc, tkc, tkg = g("T_cpu"), g("t_kvcpy_cpu"), g("t_kvcpy_gpu")
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        cpu = _f_over_s(np.full(len(fl), has_fq) & ((fl & DEV_CPU_RATE) != 0), fq, g("scpu_b1"))
        hb = (fl & DEV_GPU) != 0
        gpu = np.where(hb, _f_over_s(np.full(len(fl), has_fq) & ((fl & DEV_GPU_RATE) != 0), fq, g("sgpu_b1")), 0.0)
        tg = np.where(hb, g("T_gpu"), 1.0)
        alpha = (cpu + tkc) + (bp / Tc)
        beta = np.where(hb, ((gpu - cpu) + (tkg - tkc)) + (bp / tg - bp / Tc), 0.0)
        bcoef = np.where(cls == 1, 0.0, beta)
        xi = (g("t_ram2vram") + g("t_vram2ram")) * np.where((fl & DEV_UMA) != 0, 0.0, 1.0)
        head = np.where((fl & DEV_HEAD) != 0, 1.0, 0.0)
        bcio = bvo * head + g("c_cpu")
        sd = np.maximum(1.0, g("s_disk"))
        p_bp, p_b = bp / sd, b_layer / sd
        cst = xi + g("t_comm")
        bad = ~(np.abs(cst) < 1e300) | ~(p_bp >= 0.0) | ~(p_b >= 0.0)
        ram, swap, metal, cgpu, cuda = g("d_avail_ram"), g("swap"), g("d_avail_metal"), g("c_gpu"), g("d_avail_cuda")
        rhs_set = np.where(cls == 1, ram - bcio, np.where(cls == 2, metal - bcio - cgpu, (ram + swap) - bcio))
        has_set = (cls == 1) | (cls == 3) | ((fl & DEV_METAL_AVAIL) != 0)
        cu, mt = (fl & DEV_CUDA_OK) != 0, (fl & DEV_METAL_OK) != 0
        rhs_cu, rhs_mt = cuda - cgpu, metal - cgpu - b_out * head

        def K(rhs, on):
            """(offset, rejected) of a capacity row present where `on`."""
            okr = (bp > 0.0) & (np.abs(rhs) < 1e300)
            kk = np.ceil(-np.where(okr, rhs, 0.0) / (bp if bp > 0.0 else 1.0) - SLACK_EPS)
            okk = np.abs(kk) < 1e8
            val = np.where(on & okr & okk, kk, _NO_ROW).astype(np.int64)
            return val, on & ~(okr & okk)

        Kset, b1 = K(rhs_set, has_set)
        Kc, b2 = K(rhs_cu, cu)
        Km, b3 = K(rhs_mt, mt)
    return {"alpha": alpha, "b": bcoef, "p_bp": p_bp, "p_b": p_b, "cst": cst, "cls": cls,
            "gpu": cu | mt, "Kset": Kset, "Kvram": np.maximum(Kc, Km), "bad": bad | b1 | b2 | b3,
            "pv": np.where(cls == 2, p_b, p_bp), "own": (cls >= 1) & (cls <= 3)}


@dataclass(frozen=True)
class PlanEvalNp:
    """evaluate_plan_np's answer: the kernel's per-fleet outputs, and the plan's x / c columns when feasible."""

    status: int
    obj_value: float
    cycle: float
    bottleneck: int
    reason: int
    x: Optional[np.ndarray] = None
    c: Optional[np.ndarray] = None

    @property
    def feasible(self) -> bool:
        return self.status == STATUS_OPTIMAL


def evaluate_plan_np(table: FleetTable, model: ModelProfile, f: int, k: int, w: Sequence[int], n: Sequence[int],
                     kv_factor: float) -> PlanEvalNp:
    """The plan (k, w, n) priced on fleet f of `table`: halda_eval_plans_kernel restated with NumPy from the
    table's arrays -- status, reason, cycle and bottleneck as the kernel writes them, and
    obj_value = c.x + sum t_comm + sum xi + kappa formed as the host API forms it."""
    M = int(table.dev_off[f + 1] - table.dev_off[f])
    w, n = np.asarray(w, np.int64), np.asarray(n, np.int64)
    if w.shape != (M,) or n.shape != (M,):
        raise ValueError(f"plan of {w.shape[0] if w.ndim else 0} / {n.shape[0] if n.ndim else 0} entries for a fleet "
                         f"of {M} devices")
    k = int(k)
    inf = math.inf
    if k <= 0:
        return PlanEvalNp(STATUS_INFEASIBLE, inf, inf, -1, REASON_NO_PLAN)
    r = plan_records(table, model, f, kv_factor)
    Wk = int(model.L) // k
    W = Wk if Wk < 1_000_000 else 0
    nanx = (r["p_bp"] == inf) | ((r["p_b"] == inf) & (r["cls"] != 2))
    reason = REASON_RECORD if (r["bad"] | nanx).any() or not Wk < 1_000_000 else 0
    wok = (w >= 1) & (w <= W)
    if not wok.all():
        reason |= REASON_RANGE_W
    if int(w.sum()) != Wk:
        reason |= REASON_SUM_W
    hs, hv = r["Kset"] != _NO_ROW, r["Kvram"] != _NO_ROW
    nhi = np.where(r["gpu"], W, 0)
    nL = np.where((r["cls"] == 3) & hs, np.maximum(0, w + r["Kset"] - W), 0)
    nU = np.minimum(nhi, w)
    nU = np.where(hv, np.minimum(nU, nhi - r["Kvram"]), nU)
    setok = ~(hs & ((r["cls"] == 1) | (r["cls"] == 2))) | (np.maximum(0, w + r["Kset"]) <= W)
    if (wok & ~((n >= nL) & (n <= nU))).any():
        reason |= REASON_RANGE_N
    if (wok & (~setok | (hv & (n > nhi - r["Kvram"])))).any():
        reason |= REASON_SLACK
    if reason:
        return PlanEvalNp(STATUS_UNSUPPORTED if reason & REASON_RECORD else STATUS_INFEASIBLE, inf, inf, -1, reason)
    sc = np.maximum(0, w - np.where(r["cls"] == 3, n, 0) + r["Kset"])
    t = np.maximum(0, n + r["Kvram"])
    wd, nd_, scd, td = w.astype(np.float64), n.astype(np.float64), sc.astype(np.float64), t.astype(np.float64)
    pv = r["pv"]
    t0, tcs, tv = r["b"] * nd_, pv * scd, pv * td
    a1, a2 = r["alpha"] * wd, (r["alpha"] + r["p_bp"]) * wd
    a1, a2 = a1 + t0, a2 + t0
    a1, a2 = np.where(r["own"], a1 + tcs, a1), np.where(r["own"], a2 + tcs, a2)
    a1, a2 = a1 + tv, a2 + tv
    P, Q = a1 - (-r["cst"]), a2 - (-r["cst"])
    H = np.where(Q >= P, 0.5 * (P + Q), P)
    z = np.where(Q > P, 0.5 * (Q - P), 0.0)
    hraw = float(H.max())
    C = max(0.0, hraw)
    bott = int(np.argmax(H == hraw)) if hraw > 0.0 else -1
    N = 7 * M + 1
    x, c = np.zeros(N), np.zeros(N)
    x[:M], x[M:2 * M] = wd, nd_
    for j in (1, 2, 3):
        x[(1 + j) * M:(2 + j) * M] = np.where(r["cls"] == j, scd, 0.0)
    x[5 * M:6 * M], x[6 * M:7 * M], x[7 * M] = td, z, C
    c[:M], c[M:2 * M], c[2 * M:3 * M], c[3 * M:4 * M] = r["alpha"], r["b"], r["p_bp"], r["p_b"]
    c[4 * M:5 * M], c[5 * M:6 * M], c[7 * M] = r["p_bp"], pv, float(k - 1)
    one = _one_fleet(table, f)
    t_sum, x_sum, kappa = (float(v[0]) for v in fleet_constants(one, model))
    obj = ((float(np.vecdot(c, x)) + t_sum) + x_sum) + kappa
    return PlanEvalNp(STATUS_OPTIMAL, obj, C, bott, 0, x, c)


def _one_fleet(table: FleetTable, f: int) -> FleetTable:
    """Fleet f of `table` as a table of its own (copies of its rows)."""
    a, b = int(table.dev_off[f]), int(table.dev_off[f + 1])
    names = [fld for fld in FleetTable.__dataclass_fields__ if fld != "dev_off"]
    return FleetTable(dev_off=np.asarray([0, b - a], np.int64),
                      **{fld: np.ascontiguousarray(getattr(table, fld)[a:b]) for fld in names})


# ------------------------------------------------------------------ the GPU entries
def _plan_arrays(table: FleetTable, plans: Sequence[Optional[Plan]], allow_none: bool):
    """(k [nf], w [nd], n [nd]) int32 of one plan per fleet; None (where allowed) is k = 0, "no plan".
    ValueError on a wrong count, wrong lengths or a non-positive k."""
    nf, nd = table.n_fleets, table.n_devices
    if len(plans) != nf:
        raise ValueError(f"{len(plans)} plans for {nf} fleets")
    k = np.zeros(nf, np.int32)
    w, n = np.zeros(nd, np.int32), np.zeros(nd, np.int32)
    sizes = table.sizes()
    for f, p in enumerate(plans):
        if p is None:
            if not allow_none:
                raise ValueError(f"fleet {f}: no plan")
            continue
        pk, pw, pn = p
        M = int(sizes[f])
        if len(pw) != M or len(pn) != M:
            raise ValueError(f"fleet {f}: plan of {len(pw)} / {len(pn)} entries for {M} devices")
        if int(pk) <= 0:
            raise ValueError(f"fleet {f}: k = {pk} must be positive")
        a = int(table.dev_off[f])
        k[f] = int(pk)
        w[a:a + M], n[a:a + M] = pw, pn
    return k, w, n


def _as_plan(inc: Incumbent) -> Optional[Plan]:
    if inc is None:
        return None
    if isinstance(inc, HALDAResult):
        return int(inc.k), list(inc.w), list(inc.n)
    k, w, n = inc
    return int(k), list(w), list(n)


class _EvalBuffers:
    """Host arrays of one halda_plan_result over a table, x / c compact (every fleet's 7 M + 1 columns back
    to back)."""

    def __init__(self, table: FleetTable):
        nf = table.n_fleets
        cols = 7 * table.sizes() + 1
        self.x_off = (np.cumsum(cols) - cols).astype(np.int64)
        ext = int(cols.sum())
        self.cols = cols
        self.status, self.bottleneck, self.reason = (np.zeros(nf, np.int32) for _ in range(3))
        self.obj, self.cycle = np.zeros(nf), np.zeros(nf)
        self.x, self.c = np.zeros(ext), np.zeros(ext)
        self.res = HaldaPlanResultC(*(ptr(a) for a in (self.status, self.obj, self.cycle, self.bottleneck,
                                                       self.reason, self.x, self.c, self.x_off)))

    def evaluations(self, table: FleetTable, model: ModelProfile) -> List[PlanEvaluation]:
        """One PlanEvaluation per fleet, obj_value = c.x + sum t_comm + sum xi + kappa formed on the host as
        _batch_results forms it (np.vecdot per row length, fleet_constants)."""
        nf = table.n_fleets
        t_sum, x_sum, kappa = fleet_constants(table, model)
        obj = np.full(nf, np.inf)
        feas = self.status == STATUS_OPTIMAL
        for N in np.unique(self.cols):
            fi = np.flatnonzero(feas & (self.cols == N))
            if len(fi) == 0:
                continue
            idx = self.x_off[fi][:, None] + np.arange(int(N))[None, :]
            cx = np.vecdot(self.c[idx], self.x[idx])
            obj[fi] = ((cx + t_sum[fi]) + x_sum[fi]) + kappa[fi]
        out = []
        for f in range(nf):
            ok, rs = bool(feas[f]), int(self.reason[f])
            b = int(self.bottleneck[f])
            out.append(PlanEvaluation(ok, float(obj[f]), float(self.cycle[f]) if ok else math.inf,
                                      b if ok and b >= 0 else None, reason_names(rs), int(self.status[f]), rs))
        return out


def evaluate_table(table: FleetTable, model: ModelProfile, k: np.ndarray, w: np.ndarray, n: np.ndarray,
                   kv_factor: float, device: int = 0) -> _EvalBuffers:
    """halda_eval_plans_host of the plan arrays (int32: k per fleet, w / n in device layout) on a table."""
    ctx = get_context(device)
    buf = _EvalBuffers(table)
    fs, keep = _host_struct(table)
    k, w, n = (np.ascontiguousarray(a, np.int32) for a in (k, w, n))
    pl = HaldaPlansC(ptr(k), ptr(w), ptr(n))
    m = model_struct(model, kv_factor)
    ctx.call("halda_eval_plans_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(pl),
             ctypes.byref(buf.res))
    del keep
    return buf


def halda_evaluate_plans_batch(fleets: Sequence[Sequence[DeviceProfile]], model: ModelProfile,
                               plans: Sequence[Plan], kv_bits: str = "8bit", device: int = 0
                               ) -> List[PlanEvaluation]:
    """One plan (k, w, n) per fleet priced in ONE GPU call. ValueError (before any GPU call) on a wrong count,
    wrong lengths or a non-positive k."""
    kv_factor = kv_bits_to_factor(kv_bits)
    fleets = fleets if isinstance(fleets, (list, tuple)) else list(fleets)
    if len(plans) != len(fleets):
        raise ValueError(f"{len(plans)} plans for {len(fleets)} fleets")
    for f, (devs, p) in enumerate(zip(fleets, plans)):
        if len(p[1]) != len(devs) or len(p[2]) != len(devs):
            raise ValueError(f"fleet {f}: plan of {len(p[1])} / {len(p[2])} entries for {len(devs)} devices")
        if int(p[0]) <= 0:
            raise ValueError(f"fleet {f}: k = {p[0]} must be positive")
    if not fleets:
        return []
    table = fleet_table(fleets, model)
    k, w, n = _plan_arrays(table, [_as_plan(p) for p in plans], allow_none=False)
    return evaluate_table(table, model, k, w, n, kv_factor, device).evaluations(table, model)


def halda_evaluate_plan(devs: Sequence[DeviceProfile], model: ModelProfile, k: int, w: Sequence[int],
                        n: Sequence[int], kv_bits: str = "8bit", device: int = 0) -> PlanEvaluation:
    """The plan (k, w, n) priced on `devs`. For r = halda_solve(devs, model, kv_bits=b),
    halda_evaluate_plan(devs, model, r.k, r.w, r.n, b).obj_value == r.obj_value, bit for bit."""
    return halda_evaluate_plans_batch([list(devs)], model, [(k, w, n)], kv_bits, device)[0]


def replacement(incumbent: PlanEvaluation, inc_plan: Optional[Plan], best: Optional[HALDAResult],
                rel_tol: float = 0.0) -> Replacement:
    """The keep-or-move verdict from a priced incumbent and the new optimum."""
    if best is None:
        return Replacement(incumbent, None, -math.inf if incumbent.feasible else math.inf, 0, False)
    moved = 0 if inc_plan is None else int(sum(abs(int(a) - int(b)) for a, b in zip(best.w, inc_plan[1])))
    if not incumbent.feasible:
        return Replacement(incumbent, best, math.inf, moved, True)
    regret = incumbent.obj_value - best.obj_value
    return Replacement(incumbent, best, regret, moved, bool(regret > rel_tol * max(1.0, abs(best.obj_value))))


def solve_plans_table(table: FleetTable, model: ModelProfile, pos: List[int], k: np.ndarray, w: np.ndarray,
                      n: np.ndarray, kv_factor: float, device: int = 0) -> Tuple[FleetSolve, _EvalBuffers]:
    """One halda_solve_fleets_plans_host call on a packed table: the sweep's FleetSolve (want_x="open") and the
    incumbents' evaluation."""
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
    buf = _EvalBuffers(table)
    fs, keep = _host_struct(table)
    k, w, n = (np.ascontiguousarray(a, np.int32) for a in (k, w, n))
    pl = HaldaPlansC(ptr(k), ptr(w), ptr(n))
    karr = np.asarray(pos, np.int32)
    m = model_struct(model, kv_factor)
    ctx.call("halda_solve_fleets_plans_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), karr.ctypes.data, nk,
             ctypes.byref(pl), ctypes.byref(buf.res), ctypes.byref(r))
    del keep
    return out, buf


def _solve_and_evaluate(fleets, model, plans: List[Optional[Plan]], Ks: List[int], kv_factor: float, device: int
                        ) -> Tuple[List[Optional[HALDAResult]], List[PlanEvaluation]]:
    """halda_replace_or_keep_batch's GPU half (tests replace it): ONE halda_solve_fleets_plans_host call."""
    pos = _positive_ks(Ks)
    table = fleet_table(fleets, model)
    k, w, n = _plan_arrays(table, plans, allow_none=True)
    if not pos:
        return [None] * len(fleets), evaluate_table(table, model, k, w, n, kv_factor, device).evaluations(table, model)
    res, buf = solve_plans_table(table, model, pos, k, w, n, kv_factor, device)
    return _batch_results(table, res, pos, model), buf.evaluations(table, model)


def halda_replace_or_keep_batch(fleets: Sequence[Sequence[DeviceProfile]], model: ModelProfile,
                                incumbents: Sequence[Incumbent], rel_tol: float = 0.0, kv_bits: str = "8bit",
                                k_candidates: Optional[Iterable[int]] = None, device: int = 0) -> List[Replacement]:
    """Per fleet: the incumbent (a HALDAResult, a (k, w, n) tuple, or None for "none yet") priced on the fleet
    as it is now, the new optimum (halda_solve_batch's result), the regret, the layers that would move, and
    `replace`: true when the incumbent is infeasible and a best exists, or when regret > rel_tol *
    max(1, |best.obj_value|). One GPU call (halda_solve_fleets_plans_host)."""
    kv_factor = kv_bits_to_factor(kv_bits)
    fleets = fleets if isinstance(fleets, (list, tuple)) else list(fleets)
    if len(incumbents) != len(fleets):
        raise ValueError(f"{len(incumbents)} incumbents for {len(fleets)} fleets")
    plans = [_as_plan(p) for p in incumbents]
    for f, (devs, p) in enumerate(zip(fleets, plans)):
        if p is None:
            continue
        if len(p[1]) != len(devs) or len(p[2]) != len(devs):
            raise ValueError(f"fleet {f}: plan of {len(p[1])} / {len(p[2])} entries for {len(devs)} devices")
        if p[0] <= 0:
            raise ValueError(f"fleet {f}: k = {p[0]} must be positive")
    if not fleets:
        return []
    if k_candidates is not None and not isinstance(k_candidates, (list, tuple)):
        k_candidates = list(k_candidates)
    Ks = _batch_k_list(model, k_candidates)
    best, evals = _solve_and_evaluate(fleets, model, plans, Ks, kv_factor, device)
    return [replacement(e, p, b, rel_tol) for e, p, b in zip(evals, plans, best)]


def halda_replace_or_keep(devs: Sequence[DeviceProfile], model: ModelProfile, incumbent: Incumbent,
                          rel_tol: float = 0.0, kv_bits: str = "8bit",
                          k_candidates: Optional[Iterable[int]] = None, device: int = 0) -> Replacement:
    """halda_replace_or_keep_batch for one fleet."""
    return halda_replace_or_keep_batch([list(devs)], model, [incumbent], rel_tol, kv_bits, k_candidates, device)[0]
