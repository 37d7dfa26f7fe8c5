"""A long-lived context held to the exact oracle across interleaved calls (tests/reuse_cases.py; DESIGN.md §9,
"Long-lived contexts").

Every other GPU test compares one call, or several of one family, on a context that starts clean. Here the same
calls run in sequence on one context -- small after large, host after device, one stream after another, beside
other contexts and other host threads, and after a call the library rejected -- and every call is checked twice:

  * against the exact oracle, by the rule of test_gpu_plan_edges.check_sweep (status, c.x within 1e-9 relative,
    where the optimum is unique the w, n, s1, s2, s3 and t columns, best k, obj_value, sets);
  * bit for bit against the same call made as the first and only call on a context created for it (fresh()):
    "the answer does not depend on what ran before" is a bit promise.

Every output array starts as -7 with a guard band of GUARD entries behind it; after the call no documented
entry is -7 and the guard is intact. Where last_fleet_ms names the launch, the step asserts it, so a stale plan
fails even when it gives the right answer."""

import contextlib
import ctypes
import io
import os
import threading
import time
from functools import lru_cache

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import halda_solve
from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, FleetSolve, HaldaFleetResultC, _fleets_struct,
                                       _host_struct, fleet_table, model_struct)

from . import plan_edge_cases as pe
from . import pressure_cases as pc
from . import reuse_cases as rc
from . import test_gpu_plan_edges as tpe
from .test_gpu_bounds import GUARD

pytestmark = pytest.mark.gpu

SENTINEL = -7
OUTS = ("best_k", "obj_value", "w", "n", "obj_by_k", "status", "x", "c")
I32 = ("best_k", "w", "n", "status")
TABLE_FIELDS = ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS
CSR_KERNELS = tpe.CSR_KERNELS | {"halda_pick_kernel"}


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


class Call:
    """One shape at one batch size as a halda_solve_fleets call: the table, its device copy, the output sizes."""

    def __init__(self, shape, nf):
        sh = pe.shape(shape)
        self.cases = pe.batch(sh, nf)
        self.model = pe.model_of(sh.L)
        self.table = fleet_table([pe.devices(c) for c in self.cases], self.model)
        self.ks = list(sh.ks)
        self.karr = np.asarray(self.ks, np.int32)
        self.m = model_struct(self.model, pe.kv_factor(pe.KV))
        nd, nk = self.table.n_devices, len(self.ks)
        self.xs = 7 * int(self.table.sizes().max()) + 1
        self.sizes = {"best_k": nf, "obj_value": nf, "w": nd, "n": nd, "obj_by_k": nf * nk, "status": nf * nk,
                      "x": nf * nk * self.xs, "c": nf * nk * self.xs}
        self.fs_host, self._keep = _host_struct(self.table)
        self._dev = None

    def device_fleets(self):
        if self._dev is None:
            torch, dev = _torch()
            arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(self.table, f))).to(dev) for f in TABLE_FIELDS}
            self._dev = (arrs, _fleets_struct(self.table, lambda f: arrs[f].data_ptr()))
        return self._dev[1]

    def host_outs(self):
        return {f: np.full(n + GUARD, SENTINEL, np.int32 if f in I32 else np.float64) for f, n in self.sizes.items()}

    def device_outs(self):
        torch, dev = _torch()
        o = {f: torch.full((n + GUARD,), SENTINEL, dtype=torch.int32 if f in I32 else torch.float64, device=dev)
             for f, n in self.sizes.items()}
        torch.cuda.synchronize(dev)  # the fills run on torch's stream, the call on the caller's
        return o


class SliceCall(Call):
    """nf fleets of pressure_cases' (M, 1/16) class (seeds 0 ..) at one k of its list, on the 80-layer model: a
    batch of at most 64 fleets that needs tables (k > 1, or R + 1 > 64), so the table kernel alone, with an LDS
    slice of M (80 // k - M + 1) + M doubles."""

    def __init__(self, M, k, nf):
        self.cases = [(M, pc.S16, s, pe.KV) for s in range(nf)]
        assert all(c in pc.cases() for c in self.cases) and k in pc.ks_of(M)
        self.model = pc.our_model()
        self.table = fleet_table([pc.devices(c[2], c[0], c[1]) for c in self.cases], self.model)
        self.ks = [k]
        self.karr = np.asarray(self.ks, np.int32)
        self.m = model_struct(self.model, pc.kv_factor(pe.KV))
        self.xs = 7 * M + 1
        self.sizes = {"best_k": nf, "obj_value": nf, "w": nf * M, "n": nf * M, "obj_by_k": nf, "status": nf,
                      "x": nf * self.xs, "c": nf * self.xs}
        self.fs_host, self._keep = _host_struct(self.table)
        self._dev = None


@lru_cache(maxsize=None)
def call_of(shape, nf):
    if isinstance(shape, tuple):  # ("slice", M, k)
        return SliceCall(shape[1], shape[2], nf)
    return Call(shape, nf)


def timed_kernels(ctx):
    """The kernels of the context's last timed halda_solve_fleets launch, or None where there was none."""
    try:
        return set(ctx.last_fleet_ms())
    except RuntimeError:
        return None


def enqueue(ctx, step, stream=None, outs=None, timed=True, ks=None):
    """Make the step's call on `ctx` (device entry: asynchronous on `stream`, a torch stream or None). Returns
    (status of the call, the output arrays as they stand: NumPy arrays or device tensors)."""
    call = call_of(step.shape, step.nf)
    karr = call.karr if ks is None else np.asarray(ks, np.int32)
    ctx.set_fleets_path(step.path)
    ctx.set_timing(timed)
    if step.entry == "host":
        o = call.host_outs() if outs is None else outs
        r = HaldaFleetResultC(*[o[f].ctypes.data for f in OUTS], None)
        with ctx._lock:
            st = ctx.lib.halda_solve_fleets_host(ctx.ctx, ctypes.byref(call.m), ctypes.byref(call.fs_host),
                                                 karr.ctypes.data, len(karr), ctypes.byref(r))
        return st, o
    fs = call.device_fleets()
    o = call.device_outs() if outs is None else outs
    r = HaldaFleetResultC(*[o[f].data_ptr() for f in OUTS], None)
    with ctx._lock:
        st = ctx.lib.halda_solve_fleets(ctx.ctx, ctypes.byref(call.m), ctypes.byref(fs), karr.ctypes.data, len(karr),
                                        ctypes.byref(r), ctypes.c_void_p(stream.cuda_stream) if stream else None)
    return st, o


def collect(step, o):
    """The output arrays on the host without their guards, the guards checked (after a synchronisation)."""
    out = {}
    for f in OUTS:
        a = o[f].cpu().numpy() if hasattr(o[f], "cpu") else o[f]
        assert (a[-GUARD:] == SENTINEL).all(), (step, f, "the guard behind the array")
        out[f] = a[:-GUARD].copy()
    return out


def run(ctx, step, stream=None, outs=None):
    """The step's call on `ctx`, synchronised: (the output arrays, the kernels last_fleet_ms names -- None where
    the call made no timed launch of its own)."""
    before = timed_kernels(ctx) if step.launch == () else None
    st, o = enqueue(ctx, step, stream, outs)
    assert st == 0, (step, st, lh.last_error(ctx.lib))
    if step.entry != "host":
        torch, dev = _torch()
        torch.cuda.synchronize(dev)
    ran = timed_kernels(ctx)
    if step.launch == ():  # the resident wave: no launch, the timed events of the call before are as they were
        assert ran == before, (step, before, ran)
        ran = None
    return collect(step, o), ran


def check_launch(step, ran):
    if step.launch is None or step.launch == ():
        return
    if step.launch == pe.CSR:
        assert "halda_lower_kernel" in ran and not (ran - CSR_KERNELS), (step, ran)
    else:
        assert ran == set(step.launch), (step, ran)


def check(step, out, what):
    """A step's output arrays against the oracle (tpe.check_sweep), every documented entry written."""
    call = call_of(step.shape, step.nf)
    nf, nk = step.nf, len(call.ks)
    for f in OUTS:
        assert not (out[f] == SENTINEL).any(), (what, step, f, "an entry was never written")
    if isinstance(call, SliceCall):
        k, M = call.ks[0], call.cases[0][0]
        for f, case in enumerate(call.cases):
            assert pc.exact(case, k)[0] == 0 and out["status"][f] == lh.STATUS_OPTIMAL, (what, case, k)
            x = out["x"][f * call.xs:(f + 1) * call.xs]
            pc.check_x(x, case, k, what)
            assert pc.close(float(out["obj_value"][f]), pc.objective(case, k)) and out["best_k"][f] == k, (what, case)
            assert np.array_equal(out["w"][f * M:(f + 1) * M], x[:M]), (what, case)
        return
    res = FleetSolve(best_k=out["best_k"], obj_value=out["obj_value"], w=out["w"], n=out["n"],
                     obj_by_k=out["obj_by_k"].reshape(nf, nk), status=out["status"].reshape(nf, nk), ks=call.ks,
                     x=out["x"].reshape(nf, nk, call.xs), c=out["c"].reshape(nf, nk, call.xs))
    tpe.check_sweep(call.cases, call.table, res, f"{what}: {step.route} {step.shape} nf = {step.nf}")
    settled = res.status != lh.STATUS_OPTIMAL
    assert not res.x[settled].any() and not res.c[settled].any(), (what, step, "x / c of a non-optimal instance")


def same_bits(got, want, what):
    for f in OUTS:
        assert got[f].tobytes() == want[f].tobytes(), (what, f)


_FRESH = {}


def fresh(step):
    """The step as the first and only call on a context created for it: (outputs, kernels). Computed once."""
    key = (step.shape, step.nf, step.path, step.entry)
    if key not in _FRESH:
        torch, dev = _torch()
        ctx = lh.HaldaContext(0)
        try:
            _FRESH[key] = run(ctx, step, torch.cuda.Stream(dev) if step.entry != "host" else None)
        finally:
            ctx.close()
        for a in _FRESH[key][0].values():
            a.setflags(write=False)
    return _FRESH[key]


def run_checked(ctx, step, what, stream=None):
    out, ran = run(ctx, step, stream)
    print(f"{what}: {step.route} {step.shape} nf = {step.nf} / {step.entry}: kernels {ran and sorted(ran)}")
    check_launch(step, ran)
    check(step, out, what)
    same_bits(out, fresh(step)[0], (what, step))
    return out


# ------------------------------------------------------------------ prepared plans, group launches, Python entries
def run_plan(ctx, step, stream, group):
    """A prepared plan's launch (or a group launch over two resident tables) of the step's two fleets: the tables'
    outputs, each against the oracle (tpe.check_resident), and the kernels that ran."""
    from distilp_amd.solver.fleets import DeviceFleetTable, PlanGroup

    torch, dev = _torch()
    sh, model, cases, _ = tpe.two(step.shape)
    sets = [cases, cases[::-1]] if group else [cases]
    tabs = []
    for cs in sets:
        table = fleet_table([pe.devices(c) for c in cs], model)
        tabs.append((table, DeviceFleetTable(table, model, [1], pe.kv_factor(pe.KV), dev, want_per_k=True)))
    for _, dt in tabs:
        for v in dt.out.values():
            v.fill_(SENTINEL)
    torch.cuda.synchronize(dev)
    ctx.set_fleets_path("fused")
    ctx.set_timing(True)
    g = PlanGroup([dt for _, dt in tabs], ctx) if group else None
    try:
        if group:
            g.launch(1, 5, stream.cuda_stream)
        else:
            tabs[0][1].launch(ctx, stream.cuda_stream)
        torch.cuda.synchronize(dev)
        ran = set(ctx.last_fleet_ms())
        outs = []
        for cs, (table, dt) in zip(sets, tabs):
            tpe.check_resident(cs, table, dt, [1], f"{step.family} {step.shape}")
            outs.append({k: v.cpu().numpy() for k, v in dt.out.items()})
            assert not any((a == SENTINEL).any() for a in outs[-1].values()), (step, "an entry was never written")
    finally:
        if g is not None:
            g.close()
        for _, dt in tabs:
            dt.replan()
    return outs, ran


_FRESH_PLANS = {}


def run_plan_checked(ctx, step, stream, what):
    group = step.family == "group"
    outs, ran = run_plan(ctx, step, stream, group)
    print(f"{what}: {step.family} {step.shape}: kernels {sorted(ran)}")
    assert ran == set(step.launch), (what, step, ran)
    same_plan_bits(outs, fresh_plan(step, stream), (what, step))


def fresh_plan(step, stream):
    """run_plan's outputs as the first and only launch on a context created for it. Computed once."""
    key = (step.family, step.shape)
    if key not in _FRESH_PLANS:
        c = lh.HaldaContext(0)
        try:
            _FRESH_PLANS[key] = run_plan(c, step, stream, step.family == "group")[0]
        finally:
            c.close()
    return _FRESH_PLANS[key]


def same_plan_bits(outs, wants, what):
    for got, want in zip(outs, wants):
        for f in got:
            assert got[f].tobytes() == want[f].tobytes(), (what, f)


def run_python(step, what):
    """A Python-level entry on the default context: its result against the oracle, its route asserted."""
    ctx = lh.get_context(0)
    sh, model, cases, fleets = tpe.two(step.shape)
    if step.family == "halda_solve":
        got = []
        for case, devs in zip(cases, fleets):
            with contextlib.redirect_stdout(io.StringIO()):
                got.append(halda_solve(devs, model, k_candidates=[1], mip_gap=1e-4, plot=False, kv_bits=pe.KV))
            tpe.as_oracle(got[-1], case, what)
        return got
    ask, route = {"bounded_fused": ("auto", "fused"), "bounded_general": ("auto", "general"),
                  "bounded_tables": ("tables", "tables")}[step.route]
    boxes = tpe.move_boxes(cases, sh.L)
    got = bd.halda_solve_bounded_batch(fleets, model, boxes, k_candidates=[1], kv_bits=pe.KV, route=ask)
    assert bd.last_bounds_route(ctx) == route, (what, step, bd.last_bounds_route(ctx))
    tpe.check_bounded(cases, boxes, got, ask)
    return got


_CHANGE_LISTS = {}


def run_family(step, model, what):
    """A step of one of the other families on the default context, through the helpers (or the oracle-holding
    test body) of that family's own GPU test, on the step's case of the family's own case file."""
    from distilp_amd.solver import halda_solve_variants

    from . import test_gpu_box as tbx
    from . import test_gpu_boxes as tbs
    from . import test_gpu_budget as tbu
    from . import test_gpu_change as tch
    from . import test_gpu_pressure as tpr
    from . import test_gpu_scale as tsc
    from . import test_gpu_subsets as tss
    from . import test_gpu_variants as tv

    ctx = lh.get_context(0)
    case, route = rc.FAMILY_CASES[step.shape], step.route
    if route == "batch_and_settled":
        tpr.test_csr_pipeline_on_host_lowered_batches(ctx, case)
    elif route in ("subfleets_fused", "subfleets_expand"):
        tpe.test_leave_one_out_on_both_sides(ctx, case, route == "subfleets_fused")
    elif route == "variants_fused_and_loop":
        sh, m, cases, fleets = tpe.two(case[0])
        variants = [(m, kv) for kv in case[1]]
        tv.check_variants(fleets, variants, ks=[1], paths=((0, "fused"), (1, "loop")))
        for (_, kv), rs in zip(variants, halda_solve_variants(fleets, variants, k_candidates=[1])):
            for c, r in zip(cases, rs):
                tpe.as_oracle(r, c[:4] + (kv,), f"{what} variants {kv}")
    elif route in ("plans_fused", "plans_two_launch"):
        alone = case == "alone_r64"
        for path in ((2,) if route == "plans_fused" else (0,) if alone else (2, 0)):
            tpe.test_plans_on_both_sides(ctx, case, alone, path)
    elif route in ("boxed_fused_and_general", "boxed_tables_and_general"):
        M, k, seeds = case
        first = "fused" if route == "boxed_fused_and_general" else "tables"
        feasible, total = tbx.check_against_oracle(ctx, model, M, k, (first, "general"), seeds)
        assert feasible >= total // 2 > 0, (what, step, feasible, total)
    elif route in ("boxes_register_and_loop", "boxes_tables_and_loop"):
        tbs.test_loop_path_gives_the_fused_routes_bits(ctx, model, case)
    elif route == "boxes_tables":
        tbs.test_slices_equal_the_exact_oracle(ctx, model, *case)
    elif route == "budget":
        name, sl = case
        cases, ps = ((tbu.bu.LIST_A, tbu.bu.PS_A) if name == "A" else (tbu.bu.LIST_B, tbu.bu.PS_B))
        cases, gold = cases[sl], tbu.bu.golden()[name]
        fleets = [list(tbu.bc.devices(M, s)) for M, k, s in cases]
        incs = [(k, gold[tbu.bu.key(M, k, s)]["w0"], [0] * M) for M, k, s in cases]
        got = tbu.bg.halda_move_frontier_batch(fleets, model, incs, 2 * max(ps), tbu.KVB)
        for (M, k, s), fr in zip(cases, got):
            g = gold[tbu.bu.key(M, k, s)]
            for p in ps:
                tbu.check_point(model, None, k, g["w0"], p, fr[p], g["obj"][str(p)], tag=(what, M, k, s))
        tbu.check_frontier_prices(model, fleets, got, what)
    elif route == "change":
        name, sl = case
        if not _CHANGE_LISTS:
            _CHANGE_LISTS.update(tch.lists_of(model))
        lists, gold = _CHANGE_LISTS[name][sl], tch.cc.golden()[name]
        solved = tch.solve_cases(model, lists)
        for key, devs, keep, k, w0, ps in lists:
            for p in ps:
                tch.check_point(model, k, w0, p, solved[key][p], gold[key]["obj"][str(p)], tag=(what, name, key))
    elif route == "subsets_expand":
        tss.test_python_entries_against_the_brute_force(tss.sc.ENTRY_CASES[case])
        assert tss.ss.last_subsets_route(ctx) in ("expand", "mixed"), tss.ss.last_subsets_route(ctx)
    elif route == "subsets_fused":
        M, seed, D = case
        tss.check_frontier([tss.fleet(M, seed)], model, D, paths=(0,), sample=16, route0="fused")
    elif route == "change_subsets":
        tsc.test_scale_in_equals_the_oracle(model, *case)
    else:
        raise AssertionError(step)
    tbs.bx.set_boxes_path(ctx, 0)
    tpe.restore(ctx)


# ------------------------------------------------------------------ 1: every family, twice, on one context
def test_every_family_small_large_small_on_one_context(llama_online_model):
    """The default context -- the one every Python entry uses, and by now every earlier test of the session --
    driven through reuse_cases.passes(): the small size of every step in order, the larger size in reverse
    order, the small size again, through device and host entries alike. Every step against the oracle, its
    launch asserted and, for the C entries, its bits equal to the same call on a fresh context; a Python entry's
    result of the third pass equals the first pass's."""
    torch, dev = _torch()
    ctx = lh.get_context(0)
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    seen = {}
    try:
        tpe.restore(ctx)
        for name, steps in rc.passes():
            for step in steps:
                what = f"pass {name}"
                if step.family not in rc.PE_FAMILIES:
                    t0 = time.monotonic()
                    run_family(step, llama_online_model, what)
                    print(f"{what}: {step.family} {step.route} {step.shape}: {time.monotonic() - t0:.2f} s")
                elif step.entry == "python":
                    got = run_python(step, what)
                    assert seen.setdefault(step, got) == got, (what, step)
                elif step.family in ("plan", "group"):
                    run_plan_checked(ctx, step, streams[step.stream], what)
                else:
                    run_checked(ctx, step, what, streams[step.stream])
    finally:
        tpe.restore(ctx)


# ------------------------------------------------------------------ 2: x_zero and rejected calls
def _no_resident_context():
    """A context whose one-fleet host calls launch the sweep instead of asking the resident wave (the caller
    closes it)."""
    old = os.environ.get("HALDA_RESIDENT")
    os.environ["HALDA_RESIDENT"] = "0"
    try:
        return lh.HaldaContext(0)
    finally:
        if old is None:
            os.environ.pop("HALDA_RESIDENT", None)
        else:
            os.environ["HALDA_RESIDENT"] = old


ONE_FLEET = rc.Step("fleets", "host_resident", "no_room", 1, "fused", "host", 0, ())  # k = 40 has no room
ONE_FLEET_LAUNCHED = ONE_FLEET._replace(route="host_zero_copy", launch=None)
AFTER_REJECT = (rc.Step("fleets", "register", "no_room", 66, "fused", "device", 0, pe.REG),
                rc.Step("fleets", "kslot", "closed_k", 66, "fused", "device", 0, pe.KSLOT))  # k = 7 has no room


@pytest.mark.parametrize("resident", [True, False], ids=["resident_wave", "HALDA_RESIDENT=0"])
def test_x_zero_is_back_after_a_zero_copy_call_and_a_rejected_one(resident):
    """A zero-copy halda_solve_fleets_host call that asks for dense x / c switches the context's x_zero off (the
    host zero-fills instead); then the same call with a descending k list, which check_fleets_args rejects after
    that point; then device-entry sweeps that ask for x and c into sentinel-filled arrays on shapes with a k
    without room. Every x / c element of a non-optimal instance is zero, the optimal ones are the oracle's, and
    the thread's error text names the rejected call's reason and is unchanged by the successful calls."""
    torch, dev = _torch()
    ctx = lh.HaldaContext(0) if resident else _no_resident_context()
    one = ONE_FLEET if resident else ONE_FLEET_LAUNCHED
    try:
        run_checked(ctx, one, "zero-copy, one fleet")
        st, o = enqueue(ctx, one, ks=call_of(one.shape, one.nf).ks[::-1])
        assert st != 0, "a descending k list was accepted"
        reason = lh.last_error(ctx.lib)
        assert "ascending" in reason, reason
        collect(one, o)  # (the guards)
        stream = torch.cuda.Stream(dev)
        for step in AFTER_REJECT:
            run_checked(ctx, step, "after the rejected call", stream)
            assert lh.last_error(ctx.lib) == reason  # the last FAILURE's message: a success leaves it
        run_checked(ctx, one, "zero-copy again")
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3: path setters restored
def _bounds_state(ctx, cases, fleets, model, boxes):
    got = bd.halda_solve_bounded_batch(fleets, model, boxes, k_candidates=[1], kv_bits=pe.KV, route="auto")
    tpe.check_bounded(cases, boxes, got, "auto")
    return ctx.paths.get("bounds", 0), bd.last_bounds_route(ctx)


@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_bounds_path_is_put_back_after_every_call_and_every_error(start):
    """From each starting bounds path: route="tables" calls of halda_solve_bounded_batch, halda_replace_within
    and solve_bounded_table, and halda_solve_boxes_batch, returning normally, raising ValueError before the
    GPU call and (solve_bounded_table on a descending k list) raising after the library rejected the call
    with the path already set. After each, ctx.paths and the route of the next route="auto" call are what they
    were before; every answer is the oracle's."""
    from distilp_amd.solver.boxes import halda_solve_boxes_batch

    ctx = lh.get_context(0)
    sh, model, cases, fleets = tpe.two("alone_r65")
    boxes = tpe.move_boxes(cases, sh.L)
    M = 64
    xo = pe.exact(cases[0], 1)[1]
    inc = (1, [int(v) for v in np.rint(xo[:M])], [int(v) for v in np.rint(xo[M:2 * M])])
    table = fleet_table(fleets, model)
    lo, hi = bd.bounds_arrays(table, boxes)
    kv = pe.kv_factor(pe.KV)
    try:
        tpe.restore(ctx)
        bd.set_bounds_path(ctx, start)
        before = _bounds_state(ctx, cases, fleets, model, boxes)
        assert before == (start, {0: "general", 1: "general", 2: "general", 3: "tables"}[start]), before

        def tables():
            got = bd.halda_solve_bounded_batch(fleets, model, boxes, k_candidates=[1], kv_bits=pe.KV, route="tables")
            assert bd.last_bounds_route(ctx) == "tables"
            tpe.check_bounded(cases, boxes, got, "tables")

        def tables_bad_bounds():
            with pytest.raises(ValueError):
                bd.halda_solve_bounded_batch(fleets, model, boxes[:1], k_candidates=[1], kv_bits=pe.KV, route="tables")
            with pytest.raises(ValueError):
                bd.halda_solve_bounded_batch(fleets, model, [(b[0][:-1], b[1]) for b in boxes], k_candidates=[1],
                                             kv_bits=pe.KV, route="tables")

        def within():
            r = bd.halda_replace_within(fleets[0], model, inc, 2, kv_bits=pe.KV, route="tables")
            tpe.check_bounded(cases[:1], boxes[:1], [r.within], "replace_within")
            assert r.incumbent.feasible and pe.close(r.incumbent.obj_value, pe.objective(cases[0], 1))

        def within_bad_move():
            with pytest.raises(ValueError):
                bd.halda_replace_within(fleets[0], model, inc, -1, kv_bits=pe.KV, route="tables")

        def table_call():
            res = bd.solve_bounded_table(table, model, [1], lo, hi, kv, route="tables")
            assert bd.last_bounds_route(ctx) == "tables"
            for f, case in enumerate(cases):
                off = int(res.x_off[f])
                assert res.status[f, 0] == lh.STATUS_OPTIMAL and pe.close(float(res.obj_value[f]), pe.objective(case, 1))
                assert pe.close(float(np.dot(pe.problem(case, 1)["c"], res.x[off:off + 7 * M + 1])),
                                pe.exact(case, 1)[2])

        def table_call_rejected():
            with pytest.raises(RuntimeError, match="ascending"):
                bd.solve_bounded_table(table, model, [2, 1], lo, hi, kv, route="tables")

        def boxes_call():
            got = halda_solve_boxes_batch(fleets, model, [boxes, boxes], k_candidates=[1], kv_bits=pe.KV)
            for row in got:
                tpe.check_bounded(cases, boxes, row, "boxes")

        def boxes_bad():
            with pytest.raises(ValueError):
                halda_solve_boxes_batch(fleets, model, [boxes, boxes[:1]], k_candidates=[1], kv_bits=pe.KV)

        for fn in (tables, tables_bad_bounds, within, within_bad_move, table_call, table_call_rejected, boxes_call,
                   boxes_bad):
            fn()
            assert ctx.paths.get("bounds", 0) == start, (fn.__name__, ctx.paths)
            assert _bounds_state(ctx, cases, fleets, model, boxes) == before, (fn.__name__, start)
    finally:
        tpe.restore(ctx)


FUSED_THEN_SEG = (rc.Step("fleets", "kslot", "nf65", 66, "fused", "device", 0, pe.KSLOT),
                  rc.Step("fleets", "segment", "nf65", 66, "seg", "device", 0, pe.SEG))


def test_a_fleets_path_set_between_identical_calls_changes_the_launch():
    """Two halda_solve_fleets calls with the same argument structs on the same buffers, halda_set_fleets_path in
    between: the thread's plan cache keys on the context's path generation, so the second call runs the segment
    kernel, not the remembered k-slot plan. Then back again. Each against the oracle and a fresh context."""
    torch, dev = _torch()
    ctx = lh.HaldaContext(0)
    stream = torch.cuda.Stream(dev)
    outs = call_of("nf65", 66).device_outs()
    for step in FUSED_THEN_SEG:
        fresh(step)  # before the calls below: a fresh context's call in between would replace the thread's cached plan
    try:
        for step in FUSED_THEN_SEG + FUSED_THEN_SEG[:1]:
            for t in outs.values():
                t.fill_(SENTINEL)
            torch.cuda.synchronize(dev)
            out, ran = run(ctx, step, stream, outs)
            assert ran == set(step.launch), (step.path, ran)
            check(step, out, f"path {step.path}")
            same_bits(out, fresh(step)[0], step)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4: the LDS attribute and the occupancy cache
# twelve distinct table slices, all smaller than the prepared plan's (64 devices on 128 layers): (M, k) of the
# pressure list's 2- and 3-device classes, W = 80 // k = 80, 40, 20, 16, 10, 8, 5, 4 and 80, 40, 20, 16
LDS_SLICES = tuple(rc.Step("fleets", "tables", ("slice", M, k), 2, "fused", "device", 0, pe.TABLES)
                   for M, ks in ((2, (1, 2, 4, 5, 8, 10, 16, 20)), (3, (1, 2, 4, 5))) for k in ks)
LDS_PLAN = rc.Step("plan", "plan", "alone_r65", 2, "fused", "device", 0, pe.TABLES)


@pytest.mark.parametrize("swapped", [False, True], ids=["plan_context_first", "other_context_first"])
def test_a_large_plan_stays_launchable_after_twelve_smaller_slices_on_two_contexts(swapped):
    """A prepared plan for the table kernel at the list's largest slice, then table-kernel solves at twelve
    distinct smaller slices -- more than the occupancy cache's 8 entries -- on the plan's context and on a second
    one in the same process (the dynamic-LDS attribute is per process and only rises), then the plan again. Every
    result against the oracle and the fresh-context bits; then with the two contexts' order swapped."""
    from distilp_amd.solver.fleets import DeviceFleetTable

    torch, dev = _torch()
    slices = {(s.shape[1], 80 // s.shape[2]) for s in LDS_SLICES}
    assert len(slices) == 12 and all(M * (W - M + 1) < 64 * 65 for M, W in slices)
    for step in LDS_SLICES:
        fresh(step)
    stream = torch.cuda.Stream(dev)
    sh, model, cases, _ = tpe.two(LDS_PLAN.shape)
    table = fleet_table([pe.devices(c) for c in cases], model)
    a, b = lh.HaldaContext(0), lh.HaldaContext(0)
    dt = DeviceFleetTable(table, model, [1], pe.kv_factor(pe.KV), dev, want_per_k=True)

    def launch_plan(tag):
        for v in dt.out.values():
            v.fill_(SENTINEL)
        torch.cuda.synchronize(dev)
        a.set_timing(True)
        dt.launch(a, stream.cuda_stream)
        torch.cuda.synchronize(dev)
        assert set(a.last_fleet_ms()) == set(pe.TABLES), tag
        tpe.check_resident(cases, table, dt, [1], tag)
        return {k: v.cpu().numpy() for k, v in dt.out.items()}

    try:
        first = launch_plan("the plan, first launch")
        for ctx, name in ((b, "second context"), (a, "plan's context")) if swapped else ((a, "plan's context"),
                                                                                         (b, "second context")):
            for step in LDS_SLICES:
                run_checked(ctx, step, name, stream)
        again = launch_plan("the plan, after twelve smaller slices")
        same_plan_bits([again], [first], "the plan's two launches")
        same_plan_bits([again], fresh_plan(LDS_PLAN, stream), "the plan against a fresh context")
    finally:
        dt.replan()
        a.close()
        b.close()


# ------------------------------------------------------------------ 5: streams and slots
def test_slots_taken_over_by_smaller_gated_batches_on_ten_streams():
    """One context, ten caller streams over its eight scratch slots (reuse_cases.STREAM_STEPS): large gated
    batches fill the eight slots, register-only batches run between them, and smaller gated batches then take
    the slots over -- their table launches read flag bytes the first launch must have rewritten, on a buffer
    that holds the larger batch's. No synchronisation until the end; then every batch against the oracle and
    the fresh-context bits."""
    torch, dev = _torch()
    assert rc.N_STREAMS > rc.SLOTS
    for step in rc.STREAM_STEPS:
        fresh(step)  # (each creates and frees a context of its own: before the launches below)
    ctx = lh.HaldaContext(0)
    streams = [torch.cuda.Stream(dev) for _ in range(rc.N_STREAMS)]
    pending = []
    try:
        for step in rc.STREAM_STEPS:
            call_of(step.shape, step.nf).device_fleets()
        torch.cuda.synchronize(dev)
        for step in rc.STREAM_STEPS:
            o = call_of(step.shape, step.nf).device_outs()
            st, o = enqueue(ctx, step, streams[step.stream], o, timed=False)
            assert st == 0, (step, st, lh.last_error(ctx.lib))
            pending.append((step, o))
        torch.cuda.synchronize(dev)
        for i, (step, o) in enumerate(pending):
            out = collect(step, o)
            check(step, out, f"stream step {i}")
            same_bits(out, fresh(step)[0], (i, step))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6: the resident wave across a pinned reallocation
def test_resident_wave_across_pinned_reallocations():
    """Three times, with growing host calls: a one-fleet call puts the resident wave up, a host call larger than
    the pinned buffer follows at once (it frees and reallocates the buffer the wave just used), and a one-fleet
    call follows that. Every call against the oracle and the fresh-context bits; the one-fleet calls make no
    launch."""
    ctx = lh.HaldaContext(0)
    sizes = [rc.host_bytes(big) for _, big in rc.RESIDENT_ROUNDS]
    assert sizes == sorted(set(sizes)) and sizes[-1] > rc.K_ZERO_COPY, sizes
    try:
        for i, (one, big) in enumerate(rc.RESIDENT_ROUNDS):
            run_checked(ctx, one, f"round {i}: the wave up")
            run_checked(ctx, big, f"round {i}: pinned grows")
            run_checked(ctx, one, f"round {i}: the wave again")
    finally:
        ctx.close()


# ------------------------------------------------------------------ 7: context churn
def test_context_churn_on_fixed_buffers():
    """Twenty times: a context solves shape A on fixed device buffers through the k-slot launch and is freed; the
    next context -- as a rule at the same address -- solves shape A on the same buffers on the "seg" path. Both
    have set their path once, so the two calls' cache keys differ in nothing but the context's uid: the
    reported kernels follow the path. A plan handle that outlives its context fails with an error status."""
    torch, dev = _torch()
    a, b = FUSED_THEN_SEG
    call = call_of(a.shape, a.nf)
    fs = call.device_fleets()
    outs = call.device_outs()
    stream = torch.cuda.Stream(dev)
    for step in (a, b):
        fresh(step)  # (not between the calls below: it would replace the thread's cached plan)
    first = {}
    addresses = set()
    for i in range(20):
        for step in (a, b):
            for t in outs.values():
                t.fill_(SENTINEL)
            torch.cuda.synchronize(dev)
            ctx = lh.HaldaContext(0)
            addresses.add(ctx.ctx.value)
            h = ctypes.c_void_p()
            try:
                out, ran = run(ctx, step, stream, outs)
                assert ran == set(step.launch), (i, step.path, ran)
                r = HaldaFleetResultC(*[outs[f].data_ptr() for f in OUTS], None)
                ctx.call("halda_fleets_plan_create", ctx.ctx, ctypes.byref(call.m), ctypes.byref(fs),
                         call.karr.ctypes.data, len(call.karr), ctypes.byref(r), ctypes.byref(h))
            finally:
                ctx.close()
            assert ctx.lib.halda_fleets_plan_launch(h, ctypes.c_void_p(stream.cuda_stream)) != 0
            ctx.lib.halda_fleets_plan_free(h)
            if step.path not in first:
                check(step, out, f"churn {i} {step.path}")
                same_bits(out, fresh(step)[0], step)
                first[step.path] = out
            same_bits(out, first[step.path], (i, step.path))
    print(f"40 contexts at {len(addresses)} distinct addresses")


# ------------------------------------------------------------------ 8: threads
THREAD_STEPS = tuple(s for s in rc.SMALL if s.entry != "python")  # every C-entry step of the small pass
N_THREADS, ROUNDS = 4, 3


def _reject(ctx, i):
    """Thread i's rejected call (each a different reason): (status, the word its message must hold)."""
    call = call_of("m64_r64", 2)
    o = call.host_outs()
    r = HaldaFleetResultC(*[o[f].ctypes.data for f in OUTS], None)
    args = [ctx.ctx, ctypes.byref(call.m), ctypes.byref(call.fs_host), call.karr.ctypes.data, 1, ctypes.byref(r)]
    word = ("ascending", "n_k", "NULL ctx", "ascending")[i]
    if i in (0, 3):
        bad = np.asarray([2, 1] if i == 0 else [0], np.int32)
        args[3], args[4] = bad.ctypes.data, len(bad)
    elif i == 1:
        args[4] = 0
    else:
        args[1] = None
    with ctx._lock:
        return ctx.lib.halda_solve_fleets_host(*args), word


def test_four_threads_four_contexts_and_two_threads_on_the_default_context():
    """Four host threads, each with its own context, started together: each runs its own rotation of the small
    pass's C-entry steps three times, makes one rejected call and reads its own reason back (the error text is
    thread_local, as the plan cache is). Every result equals the single-threaded bits and the oracle. Then two
    threads alternate halda_solve and halda_solve_bounded(route="tables") on the shared default context; each
    answer equals the single-threaded one. A join that outlasts ten times the single-threaded time ends the
    session (nothing further starts on the GPU)."""
    torch, dev = _torch()
    t0 = time.monotonic()
    main_stream = torch.cuda.Stream(dev)
    for step in THREAD_STEPS:  # single-threaded: the bits, the device copies of the tables
        if step.family in ("plan", "group"):
            fresh_plan(step, main_stream)  # (held to the oracle inside)
        else:
            check(step, fresh(step)[0], "single-threaded")
    single = time.monotonic() - t0
    limit = 10.0 * ROUNDS * max(single, 0.5)
    barrier = threading.Barrier(N_THREADS)
    results, errors = [[] for _ in range(N_THREADS)], []

    def worker(i):
        ctx = None
        try:
            ctx = lh.HaldaContext(0)
            stream = torch.cuda.Stream(dev)
            order = THREAD_STEPS[i:] + THREAD_STEPS[:i]
            barrier.wait(limit)
            for rnd in range(ROUNDS):
                for step in order:
                    if step.family in ("plan", "group"):
                        out, ran = run_plan(ctx, step, stream, step.family == "group")
                        assert ran == set(step.launch), (step, ran)
                    else:
                        out, ran = run(ctx, step, stream)
                        check_launch(step, ran)
                    results[i].append((step, out))
                if rnd == 1:
                    st, word = _reject(ctx, i)
                    assert st != 0, (i, "the call was accepted")
                    results[i].append(("reason", word))
            barrier.wait(limit)  # every thread has failed once by now: each still reads its own text
            results[i].append(("text", lh.last_error(ctx.lib)))
        except BaseException as e:  # noqa: BLE001 -- handed to the main thread
            errors.append((i, repr(e)))
            barrier.abort()
        finally:
            if ctx is not None:
                ctx.close()

    def join_all(threads):
        for t in threads:
            t.start()
        for t in threads:
            t.join(limit)
            if t.is_alive():
                pytest.exit(f"test_gpu_reuse: a thread did not finish within {limit:.0f} s", returncode=3)

    join_all([threading.Thread(target=worker, args=(i,), daemon=True) for i in range(N_THREADS)])
    assert not errors, errors
    for i, got in enumerate(results):
        word = next(v for k, v in got if k == "reason")
        text = next(v for k, v in got if k == "text")
        assert word in text, (i, word, text)
        runs = [(k, v) for k, v in got if k not in ("reason", "text")]
        assert len(runs) == ROUNDS * len(THREAD_STEPS)
        for step, out in runs:  # (held to the oracle above)
            if step.family in ("plan", "group"):
                same_plan_bits(out, fresh_plan(step, main_stream), (i, step))
            else:
                same_bits(out, fresh(step)[0], (i, step))

    # two threads, one context: the Python entries take the context's lock
    ctx = lh.get_context(0)
    sh, model, cases, fleets = tpe.two("alone_r65")
    boxes = tpe.move_boxes(cases, sh.L)

    def solve():
        with contextlib.redirect_stdout(io.StringIO()):
            return halda_solve(fleets[1], model, k_candidates=[1], mip_gap=1e-4, plot=False, kv_bits=pe.KV)

    def bounded():
        return bd.halda_solve_bounded(fleets[0], model, *boxes[0], k_candidates=[1], kv_bits=pe.KV, route="tables")

    try:
        tpe.restore(ctx)
        want = {"solve": solve(), "bounded": bounded()}
        tpe.as_oracle(want["solve"], cases[1], "halda_solve")
        tpe.check_bounded(cases[:1], boxes[:1], [want["bounded"]], "tables")
        got, errors2 = {"solve": [], "bounded": []}, []
        pair = threading.Barrier(2)

        def alternate(name, fn):
            try:
                pair.wait(limit)
                for _ in range(5):
                    got[name].append(fn())
            except BaseException as e:  # noqa: BLE001
                errors2.append((name, repr(e)))
                pair.abort()

        # (redirect_stdout is process-wide: halda_solve's thread prints nothing with plot=False either way)
        join_all([threading.Thread(target=alternate, args=(n, f), daemon=True)
                  for n, f in (("solve", solve), ("bounded", bounded))])
        assert not errors2, errors2
        for name in got:
            assert len(got[name]) == 5 and all(r == want[name] for r in got[name]), name
        assert ctx.paths.get("bounds", 0) == 0
    finally:
        tpe.restore(ctx)
