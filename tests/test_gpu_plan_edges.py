"""Both sides of every integer threshold of the fused sweep's launch plan (tests/plan_edge_cases.py), each
against the exact oracle: status, c.x within 1e-9 relative, where the oracle's optimum is unique the w, n, s1,
s2, s3 and t columns of x, the sweep's best k (strict "<") and obj_value, and sets. Every test also asserts the
launch itself -- the kernels that ran and those that did not (last_fleet_ms with timing on), the LDS shape
(halda_lds_bytes), or the module's own route accessor -- so a shape that drifts to the other side of its
threshold fails here rather than passing on another kernel ("Plan edges").

sweep, check_sweep and check_resident are those of test_gpu_irregular.py, reading the cases of this list."""

import contextlib
import io
from functools import lru_cache

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import halda_solve, halda_solve_batch
from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import fleet_table, open_x_offsets, solve_table
from oracle import milp_oracle as mo

from . import plan_edge_cases as pe

pytestmark = pytest.mark.gpu

CSR_KERNELS = {"halda_lower_kernel", "halda_screen_kernel", "halda_solve_k1_kernel", "halda_solve_kernel"}


@pytest.fixture(scope="module")
def ctx():
    c = lh.get_context(0)
    yield c
    restore(c)


def restore(c):
    c.set_fleets_path("fused")
    c.set_timing(False)
    pl.set_plans_path(c, 0)
    bd.set_bounds_path(c, 0)


def sweep(ctx, sh, nf, path="fused", want_x=True):
    """solve_table of the shape's batch of nf fleets over its k list, and the kernels that ran."""
    cases = pe.batch(sh, nf)
    model = pe.model_of(sh.L)
    table = fleet_table([pe.devices(c) for c in cases], model)
    ctx.set_fleets_path(path)
    ctx.set_timing(True)
    try:
        res = solve_table(table, model, list(sh.ks), pe.kv_factor(pe.KV), want_x=want_x)
        ran = set(ctx.last_fleet_ms())
    finally:
        ctx.set_fleets_path("fused")
        ctx.set_timing(False)
    return cases, table, res, ran


def check_sweep(cases, table, res, what):
    """A FleetSolve (dense x) against the oracle: per (fleet, k) the status, x and obj_by_k -- a k without room
    INFEASIBLE with an all-zero x; per fleet the best k by the reference's strict "<", obj_value and (w, n)."""
    for f, case in enumerate(cases):
        M, L = case[0], case[3]
        a = int(table.dev_off[f])
        best = None
        for j, k in enumerate(res.ks):
            if L // k < M:
                assert res.status[f, j] == lh.STATUS_INFEASIBLE and np.isinf(res.obj_by_k[f, j]), (what, case, k)
                assert not res.x[f, j].any(), (what, case, k, "x of a settled k")
                continue
            st = pe.exact(case, k)[0]
            assert st == 0, (what, case, k, st)  # every instance with room is feasible (tests/test_plan_edges.py)
            assert res.status[f, j] == lh.STATUS_OPTIMAL, (what, case, k, res.status[f, j])
            x = res.x[f, j, :7 * M + 1]
            pe.check_x(x, case, k, what)
            obj = mo.objective_value(pe.problem(case, k), x)
            assert pe.close(float(res.obj_by_k[f, j]), obj) and pe.close(obj, pe.objective(case, k)), (
                what, case, k, float(res.obj_by_k[f, j]), obj, pe.objective(case, k))
            if best is None or obj < best[0]:
                best = (obj, k, x)
        assert best is not None and res.best_k[f] == best[1], (what, case, int(res.best_k[f]), best[1])
        assert pe.close(float(res.obj_value[f]), best[0]), (what, case)
        assert np.array_equal(res.w[a:a + M], best[2][:M]) and np.array_equal(res.n[a:a + M], best[2][M:2 * M]), (
            what, case)
        if pe.best_k_is_clear(case, res.ks):
            assert res.best_k[f] == pe.best_k(case, res.ks)[0], (what, case, int(res.best_k[f]))
        assert table.sets(f) == mo.sets_of(pe.devices(case)), (what, case)


def same_answers(a, b, what):
    for f in ("status", "best_k", "w", "n"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)


def as_oracle(r, case, what=""):
    """A HALDAResult of a case's fleet against the oracle at k = 1: obj_value, sets and, where unique, w, n."""
    M = case[0]
    assert pe.exact(case, 1)[0] == 0
    assert r is not None and r.k == 1 and pe.close(r.obj_value, pe.objective(case, 1)), (what, case, r)
    assert r.sets == mo.sets_of(pe.devices(case)), (what, case)
    if pe.unique(case, 1):
        xo = pe.exact(case, 1)[1]
        assert r.w == [int(v) for v in xo[:M]] and r.n == [int(v) for v in xo[M:2 * M]], (what, case, r)


def params(part):
    return [pytest.param(sh.name, nf, id=f"{sh.name}-nf{nf}") for sh in pe.STATIC_SHAPES if sh.part == part
            for nf in sh.launch]


# ------------------------------------------------------------------ A: the 64-lane gate
@pytest.mark.parametrize("name,nf", params("A"))
def test_the_64_lane_gate(ctx, name, nf):
    """k = 1 alone at R + 1 = 64 (the register launch alone, every DP lane in use) and at 65 (the table kernel
    alone for at most 64 fleets, the register launch with the gated table launch behind it for more), on the
    default path and with the exact DP forced for every k = 1 solve: at 64 "dp" runs k1_dp on all 64 lanes, at
    65 it flags every instance, so the gated table launch redoes the whole batch."""
    sh = pe.shape(name)
    assert pe.predicate(sh, nf) == (sh.side == "at")
    runs = {}
    try:
        for path in ("fused", "dp"):
            cases, table, res, ran = sweep(ctx, sh, nf, path)
            print(f"{name} nf = {nf} / {path}: kernels {sorted(ran)}")
            assert ran == set(sh.launch[nf]), (name, nf, path, ran)
            check_sweep(cases, table, res, f"{name} nf = {nf} / {path}")
            runs[path] = res
        same_answers(runs["dp"], runs["fused"], (name, nf))
    finally:
        restore(ctx)


# ------------------------------------------------------------------ B: the k-slot kernel's edges
@pytest.mark.parametrize("name,nf", params("B"))
def test_the_kslot_and_segment_kernels_edges(ctx, name, nf):
    """The batch size (64: the table kernel alone; 65, 66, 67: the k-slot kernel, its last workgroup holding 1,
    2 and 3 fleets), the slot count (16 open k: k-slot; 17: the table kernel), a single table slot (the extra
    wave of part 2) and one helper slot, no k > 1 with room (the register launch alone, k = 40 INFEASIBLE), a
    non-divisor k next to a settled one, and the k-slot launch's LDS (k = 2, 3 on 200 layers fit it; with k = 4
    they do not and the segment kernel runs). Four paths, each against the oracle and each with its launch
    asserted as the exact set of kernels that ran: the default; the split in sequential order (the same plan);
    "seg", which turns the k-slot kernel off, so the segment kernel takes the same batches -- more than 64
    fleets, at most 16 k, a last wave of 1, 2 and 3 segments -- and hands 17 k or 64 fleets to the table
    kernel; and the forced DP, which plans with neither. Status, best k, w and n are equal across the four."""
    sh = pe.shape(name)
    assert pe.predicate(sh, nf) == (sh.side == "at")
    want = {"fused": sh.launch[nf], "kslot_sequential": sh.launch[nf], "seg": sh.seg[nf], "dp": sh.dp[nf]}
    runs = {}
    try:
        for path in ("fused", "kslot_sequential", "seg", "dp"):
            cases, table, res, ran = sweep(ctx, sh, nf, path)
            print(f"{name} nf = {nf} / {path}: kernels {sorted(ran)}")
            assert ran == set(want[path]), (name, nf, path, ran)
            check_sweep(cases, table, res, f"{name} nf = {nf} / {path}")
            runs[path] = res
        for path in ("kslot_sequential", "seg", "dp"):
            same_answers(runs[path], runs["fused"], (name, nf, path))
        if any(sh.L // k < max(sh.sizes) for k in sh.ks):
            # the settled k in the compact layout: no x at all (x_off == -1), the others' x as above
            cases, table, res, _ = sweep(ctx, sh, nf, want_x="open")
            want_off = open_x_offsets(table, pe.model_of(sh.L), list(sh.ks))
            assert np.array_equal(res.x_off, want_off)
            nk, settled = len(sh.ks), 0
            for f, case in enumerate(cases):
                for j, k in enumerate(sh.ks):
                    off = int(res.x_off[f * nk + j])
                    if sh.L // k < case[0]:
                        assert off == -1 and res.status[f, j] == lh.STATUS_INFEASIBLE, (name, case, k)
                        settled += 1
                        continue
                    assert res.status[f, j] == lh.STATUS_OPTIMAL, (name, case, k)
                    pe.check_x(res.x[off:off + 7 * case[0] + 1], case, k, f"{name} open x")
            assert settled >= nf
            same_answers(res, runs["fused"], (name, nf, "open x"))
    finally:
        restore(ctx)


# ------------------------------------------------------------------ C: the k-count gate
def test_the_k_count_gate(ctx):
    """64 k stay on the fused sweep (no CSR kernel), 65 k go through the CSR pipeline (halda_lower_kernel):
    both against the oracle per k, and equal status, w and n columns on the shared 64 k."""
    runs = {}
    try:
        for name in ("k64", "k65"):
            sh = pe.shape(name)
            (nf, launch), = sh.launch.items()
            assert pe.predicate(sh, nf) == (sh.side == "at")
            cases, table, res, ran = sweep(ctx, sh, nf)
            print(f"{name}: kernels {sorted(ran)}")
            if name == "k64":
                assert ran == set(launch) and not (ran & CSR_KERNELS), ran
            else:
                assert "halda_lower_kernel" in ran and not (ran - CSR_KERNELS - {"halda_pick_kernel"}), ran
            check_sweep(cases, table, res, name)
            runs[name] = (cases, res)
        (c64, r64), (c65, r65) = runs["k64"], runs["k65"]
        assert c64 == c65 and r65.ks[:64] == r64.ks
        M = 2
        assert np.array_equal(r65.status[:, :64], r64.status)
        assert np.array_equal(r65.x[:, :64, :2 * M], r64.x[:, :, :2 * M])
    finally:
        restore(ctx)


# ------------------------------------------------------------------ D: the LDS budget
@pytest.mark.parametrize("name", ["lds_fits", "lds_over"])
def test_the_lds_budget(ctx, name):
    """66-device fleets (wider than a wave: tables from the start) at the largest L whose table slice fits
    160 KiB -- the table kernel alone on LDS tables -- and at the next L -- the register launch, which flags
    every fleet, plus the global-table launch (reported in the table kernel's slot, include/halda.h)."""
    sh = pe.shape(name)
    (nf, launch), = sh.launch.items()
    M, r1 = 66, sh.L - 66 + 1
    lds = ctx.lib.halda_lds_bytes(7 * (M - 1) + 1, r1, M * r1, 0)
    below = ctx.lib.halda_lds_bytes(7 * (M - 1) + 1, r1 - 1, M * (r1 - 1), 0)
    above = ctx.lib.halda_lds_bytes(7 * (M - 1) + 1, r1 + 1, M * (r1 + 1), 0)
    print(f"{name}: L = {sh.L}, LDS slice {lds} B (L - 1: {below} B, L + 1: {above} B)")
    if name == "lds_fits":
        assert lds <= pe.LDS_BUDGET < above
    else:
        assert below <= pe.LDS_BUDGET < lds
    assert pe.predicate(sh, nf) == (sh.side == "at")
    runs = {}
    try:
        for path in ("fused", "dp"):
            cases, table, res, ran = sweep(ctx, sh, nf, path)
            print(f"{name} / {path}: kernels {sorted(ran)}")
            assert ran == set(launch), (name, path, ran)
            check_sweep(cases, table, res, f"{name} / {path}")
            runs[path] = res
        same_answers(runs["dp"], runs["fused"], name)
    finally:
        restore(ctx)


# ------------------------------------------------------------------ E: what hangs on the register launch alone
SIDES = [("alone_r64", True), ("alone_r65", False)]


def two(name):
    """(shape, model, cases, fleets) of a two-fleet shape."""
    sh = pe.shape(name)
    cases = pe.cases_of(sh)
    return sh, pe.model_of(sh.L), cases, [pe.devices(c) for c in cases]


@pytest.mark.parametrize("name,alone", [("loo_r64", True), ("loo_r65", False)])
def test_leave_one_out_on_both_sides(ctx, name, alone):
    """halda_leave_one_out_batch of two 64-device fleets, k = 1: their 63-device lists sit at R + 1 = 64 on 126
    layers (the sub-fleet kernel, "fused") and at 65 on 127 (the expansion route). Only eight of each fleet's 64
    lists (pe.LOO_DROPS) are held to the exact oracle -- the oracle's time is the budget; the other 56 are only
    compared with halda_solve_batch of the materialised lists (pydantic ==), which is another GPU path."""
    from distilp_amd.solver.subfleets import halda_leave_one_out_batch, last_subfleets_route

    sh = pe.shape(name)
    assert pe.predicate(sh, 0) == alone
    model = pe.model_of(sh.L)
    parents = {(c[1], c[2]): pe.pc.devices(c[2], 64, c[1]) for c in pe.cases_of(sh)}
    try:
        got = halda_leave_one_out_batch(list(parents.values()), model, k_candidates=[1], kv_bits=pe.KV)
        assert last_subfleets_route(ctx) == ("fused" if alone else "expand"), last_subfleets_route(ctx)
        for (key, devs), rs in zip(parents.items(), got):
            lists = [devs[:i] + devs[i + 1:] for i in range(64)]
            assert rs == halda_solve_batch(lists, model, k_candidates=[1], kv_bits=pe.KV), (name, key)
            for case in pe.cases_of(sh):
                if (case[1], case[2]) == key:
                    as_oracle(rs[case[5]], case, name)
    finally:
        restore(ctx)


@pytest.mark.parametrize("name,alone", SIDES)
def test_variants_on_both_sides(ctx, name, alone):
    """halda_solve_variants over kv 4bit / 8bit / fp16 at R + 1 = 64 (the variants kernel) and at 65 (the table
    variants kernel): bit for bit one halda_solve_fleets call per variant (check_variants, which asserts the
    route), and every variant's every fleet against the exact oracle at that kv width."""
    from distilp_amd.solver import halda_solve_variants

    from .test_gpu_variants import check_variants

    sh, model, cases, fleets = two(name)
    assert pe.predicate(sh, 2) == alone
    variants = [(model, "4bit"), (model, "8bit"), (model, "fp16")]
    try:
        check_variants(fleets, variants, ks=[1], paths=((0, "fused"),))
        ctx.set_timing(True)
        got = halda_solve_variants(fleets, variants, k_candidates=[1])
        ran = set(ctx.last_fleet_ms())
        print(f"variants {name}: kernels {sorted(ran)}")
        assert ran == set(sh.launch[2]), ran  # reported in the register / table kernel's slot
        for (_, kv), rs in zip(variants, got):
            for case, r in zip(cases, rs):
                as_oracle(r, case[:4] + (kv,), f"variants {name} {kv}")
    finally:
        restore(ctx)


@pytest.mark.parametrize("path", [2, 0])
@pytest.mark.parametrize("name,alone", SIDES)
def test_plans_on_both_sides(ctx, name, alone, path):
    """halda_solve_fleets_plans on plans path 2 (one fused launch at R + 1 = 64, two launches at 65) and on the
    default path (two launches): the sweep against the oracle, the evaluation of the oracle's own optimum at the
    oracle's objective and of a neighbour plan against evaluate_plan_np."""
    sh, model, cases, fleets = two(name)
    M = 64
    table = fleet_table(fleets, model)
    rng = np.random.default_rng(pe.pc.NEIGHBOUR_SEED)
    plans = []
    for f, c in enumerate(cases):
        xo = pe.exact(c, 1)[1]
        w, n = [int(v) for v in np.rint(xo[:M])], [int(v) for v in np.rint(xo[M:2 * M])]
        plans.append((1, w, n) if f == 0 else (1,) + tuple(pe.pc.neighbours(rng, w, n)[0][1:]))
    k, w, n = pl._plan_arrays(table, plans, allow_none=False)
    try:
        pl.set_plans_path(ctx, path)
        res, buf = pl.solve_plans_table(table, model, [1], k, w, n, pe.kv_factor(pe.KV))
        route = pl.last_plans_route(ctx)
        print(f"plans {name} path {path}: route {route}")
        assert route == ("fused" if path == 2 and alone else "two_launch"), route
        for f, case in enumerate(cases):
            e = pl.evaluate_plan_np(table, model, f, *plans[f], pe.kv_factor(pe.KV))
            assert (buf.status[f], buf.reason[f], buf.bottleneck[f]) == (e.status, e.reason, e.bottleneck), (case, e)
            if e.feasible:
                assert buf.cycle[f] == e.cycle and pe.close(float(buf.obj[f]), e.obj_value), case
            if f == 0:
                assert e.feasible and pe.close(float(buf.obj[f]), pe.objective(case, 1)), case
            off = int(res.x_off[f])
            assert res.status[f, 0] == lh.STATUS_OPTIMAL and res.best_k[f] == 1, case
            pe.check_x(res.x[off:off + 7 * M + 1], case, 1, f"plans {name} path {path}")
            assert pe.close(float(res.obj_value[f]), pe.objective(case, 1)), case
    finally:
        restore(ctx)


def move_boxes(cases, W, D=2):
    """Per case the (w_min, w_max) of the D-layer move box around the oracle's k = 1 optimum."""
    boxes = []
    for case in cases:
        w0 = [int(v) for v in np.rint(pe.exact(case, 1)[1][:case[0]])]
        boxes.append(([max(1, v - D) for v in w0], [min(W, v + D) for v in w0]))
    return boxes


@lru_cache(maxsize=None)
def _boxed_exact(case, lo, hi):
    """(the dense k = 1 problem of `case` with the w columns' bounds narrowed, the exact oracle's answer)."""
    M = case[0]
    p = dict(pe.problem(case, 1))
    p["lb"], p["ub"] = p["lb"].copy(), p["ub"].copy()
    p["lb"][:M], p["ub"][:M] = lo, hi
    return p, mo.exact_solve(p)


def check_bounded(cases, boxes, got, ask):
    """halda_solve_bounded_batch's results at k = 1 against the exact oracle on the dense problem with the w
    columns' bounds narrowed to the boxes."""
    for case, (lo, hi), r in zip(cases, boxes, got):
        M = case[0]
        p, (st, xo, b1, b2, _) = _boxed_exact(case, tuple(lo), tuple(hi))
        assert st == 0, (case, st)  # the move box around the optimum holds the optimum
        assert r is not None and r.k == 1, (case, ask)
        assert pe.close(r.obj_value, mo.objective_value(p, xo)), (case, ask, r.obj_value)
        assert pe.close(r.obj_value, pe.objective(case, 1)), (case, ask)
        assert all(a <= v <= b for a, v, b in zip(lo, r.w, hi)), (case, ask)
        if mo.uniqueness_margin_ok(b1, b2):
            assert r.w == [int(v) for v in xo[:M]] and r.n == [int(v) for v in xo[M:2 * M]], (case, ask, r)


@pytest.mark.parametrize("name,alone", SIDES)
def test_bounded_sweep_on_both_sides(ctx, name, alone):
    """halda_solve_bounded_batch within the D = 2 move box around the oracle's optimum: the fused bounded sweep
    at R + 1 = 64; at 65 the general route ("auto") and the table route: each against the exact oracle on the
    dense problem with the w columns' bounds narrowed."""
    sh, model, cases, fleets = two(name)
    boxes = move_boxes(cases, sh.L)
    try:
        for ask, route in ((("auto", "fused"),) if alone else (("auto", "general"), ("tables", "tables"))):
            got = bd.halda_solve_bounded_batch(fleets, model, boxes, k_candidates=[1], kv_bits=pe.KV, route=ask)
            assert bd.last_bounds_route(ctx) == route, (ask, bd.last_bounds_route(ctx))
            check_bounded(cases, boxes, got, ask)
    finally:
        restore(ctx)


def check_resident(cases, table, dt, ks, what):
    """A resident table's outputs (no x) against the oracle: status, obj_by_k, best k, obj_value, (w, n)."""
    out = {k: v.cpu().numpy() for k, v in dt.out.items()}
    nk = len(ks)
    for f, case in enumerate(cases):
        M, a = case[0], int(table.dev_off[f])
        for j, k in enumerate(ks):
            assert case[3] // k >= M and pe.exact(case, k)[0] == 0
            assert out["status"][f * nk + j] == lh.STATUS_OPTIMAL, (what, case, k)
            assert pe.close(float(out["obj_by_k"][f * nk + j]), pe.objective(case, k)), (what, case, k)
        kb, ob = pe.best_k(case, ks)
        assert pe.close(float(out["obj_value"][f]), ob), (what, case)
        if pe.best_k_is_clear(case, ks):
            assert out["best_k"][f] == kb, (what, case, int(out["best_k"][f]), kb)
            if pe.unique(case, kb):
                xo = pe.exact(case, kb)[1]
                assert np.array_equal(out["w"][a:a + M], xo[:M]) and np.array_equal(out["n"][a:a + M], xo[M:2 * M]), (
                    what, case)


@pytest.mark.parametrize("name,alone", SIDES)
def test_group_launch_on_both_sides(ctx, name, alone):
    """PlanGroup over two resident tables: one persistent steps launch at R + 1 = 64 (reported in the register
    kernel's slot), batch by batch through the table kernel at 65; every table's outputs against the oracle."""
    import torch

    from distilp_amd.solver.fleets import DeviceFleetTable, PlanGroup

    sh, model, cases, _ = two(name)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    sets = [cases, cases[::-1]]
    tabs = []
    for cs in sets:
        table = fleet_table([pe.devices(c) for c in cs], model)
        tabs.append((table, DeviceFleetTable(table, model, [1], pe.kv_factor(pe.KV), dev, want_per_k=True)))
    group = PlanGroup([dt for _, dt in tabs], ctx)
    try:
        assert group.persistent == alone
        for _, dt in tabs:
            for v in dt.out.values():
                v.zero_()
        torch.cuda.synchronize(dev)
        ctx.set_timing(True)
        group.launch(1, 5, stream.cuda_stream)
        torch.cuda.synchronize(dev)
        ran = set(ctx.last_fleet_ms())
        print(f"group launch {name}: persistent {group.persistent}, kernels {sorted(ran)}")
        assert ran == set(sh.launch[2]), ran
        for cs, (table, dt) in zip(sets, tabs):
            check_resident(cs, table, dt, [1], f"group {name}")
    finally:
        group.close()
        restore(ctx)


@pytest.mark.parametrize("name,alone", SIDES)
def test_halda_solve_on_both_sides(ctx, name, alone):
    """One halda_solve per fleet: through the resident wave at R + 1 = 64 (no launch: the timed events of the
    sweep before it, a two-launch one, are left as they were), through a launch of the table kernel at 65."""
    sh, model, cases, fleets = two(name)
    marker = pe.shape("m2_r65")  # 66 two-device fleets: the register launch and the gated table launch
    try:
        for case, devs in zip(cases, fleets):
            assert sweep(ctx, marker, 66)[3] == set(pe.REG_GATED)
            ctx.set_timing(True)
            before = ctx.last_fleet_ms()
            with contextlib.redirect_stdout(io.StringIO()):
                r = halda_solve(devs, model, k_candidates=[1], mip_gap=1e-4, plot=False, kv_bits=pe.KV)
            after = ctx.last_fleet_ms()
            print(f"halda_solve {name}: before {sorted(before)}, after {sorted(after)}")
            if alone:
                assert after == before and set(before) == set(pe.REG_GATED), (name, before, after)
            else:
                assert set(after) == set(pe.TABLES), (name, before, after)
            as_oracle(r, case, f"halda_solve {name}")
    finally:
        restore(ctx)
