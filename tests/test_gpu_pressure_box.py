"""Layer bounds on w and n under memory pressure and on irregular fleets (tests/pressure_box_cases.py), on every
route of halda_solve_fleets_boxed -- the fused launch (halda_sweep_box_kernel), the table launch
(halda_sweep_box_tables_kernel) and the general route (halda_box_cols_kernel, then the CSR pipeline) -- each
against the exact oracle: status, objective within 1e-9 relative, (w, n) inside the box and, where the optimum is
unique, the w, n, s1, s2, s3 and t columns of x. No fleet of tests/box_cases.py has t > n or a positive set-row lower
end, so an n_max that narrowed the VRAM slack t with n changes nothing there; on the tight fleets of this list it
turns feasible instances infeasible. The routes agree with each other within 1e-12, pins price the
plan as halda_eval_plans does, an n box that never binds gives the w-only call's bits, the DP test path gives the
greedy's answers, and the Python entries equal the oracle. No shape takes both the fused and the table route
(path 3 takes the fused launch wherever its gate holds), so those two are not compared with each other."""

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import halda_replace_within, halda_solve_bounded
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import fleet_table

from . import box_cases as xc
from . import pressure_box_cases as pb
from . import pressure_cases as pc
from .test_gpu_bounds import KV, same
from .test_gpu_box import BoxRun, close_outputs, launched, on_route

pytestmark = pytest.mark.gpu

L = pc.L


@pytest.fixture
def ctx():
    c = lh.get_context(0)
    yield c
    c.set_fleets_path("fused")
    c.set_timing(False)
    bd.set_bounds_path(c, 0)


def batch(M, k, kinds, fleet_list=None):
    """The instances of (M, k) that exist as one table: [(fleet, kind)], the BoxRun and the flat box arrays."""
    model = pc.our_model()
    inst = [(f, kind) for f in (pb.fleets(M) if fleet_list is None else fleet_list) for kind in kinds
            if pb.box(f, k, kind) is not None]
    assert all(pb.model_of(f) is model for f, _ in inst)
    table = fleet_table([pb.devices(f) for f, _ in inst], model)
    boxes = [pb.box(f, k, kind) for f, kind in inst]
    return inst, BoxRun(table, model, [k]), xc.flat(boxes, table), table


def check_against_oracle(got, inst, run, M, k, what):
    """One route's outputs of a batch against pressure_box_cases.answer; the number of feasible instances."""
    N, feasible = 7 * M + 1, 0
    for i, (f, kind) in enumerate(inst):
        b, st, x, _, obj, unique = pb.answer(f, k, kind)
        tag = (what, f, k, kind)
        if st != 0:
            assert got["status"][i] == lh.STATUS_INFEASIBLE and got["best_k"][i] == 0, tag
            assert got["obj_value"][i] == np.inf, tag
            continue
        feasible += 1
        assert got["status"][i] == lh.STATUS_OPTIMAL and got["best_k"][i] == k, tag
        assert pc.close(float(got["obj_value"][i]), obj), tag + (float(got["obj_value"][i]), obj)
        assert got["obj_by_k"][i] == got["obj_value"][i], tag
        a = i * M
        w, n = got["w"][a:a + M], got["n"][a:a + M]
        assert (w >= b[0]).all() and (w <= b[1]).all() and (n >= b[2]).all() and (n <= b[3]).all(), tag
        assert w.sum() == L // k and (n <= w).all(), tag
        gx = got["x"][i * run.xs:i * run.xs + N]
        assert np.array_equal(gx[:M], w) and np.array_equal(gx[M:2 * M], n), tag
        pb.check_x(gx, f, k, kind, what)
        if unique:
            assert w.tolist() == [int(v) for v in np.rint(x[:M])], tag
            assert n.tolist() == [int(v) for v in np.rint(x[M:2 * M])], tag
    return feasible


# ------------------------------------------------------------------ 1. every kind on every route, against the oracle
@pytest.mark.parametrize("M,k,routes", [(64, 1, ("fused", "general")), (16, 1, ("tables", "general")),
                                        (16, 2, ("tables", "general")), (16, 4, ("tables", "general")),
                                        (5, 1, ("tables", "general")), (5, 2, ("tables", "general")),
                                        (5, 4, ("tables", "general"))])
def test_boxes_under_pressure_equal_the_oracle_on_every_route(ctx, M, k, routes):
    inst, run, flat, _ = batch(M, k, pb.KINDS)
    outs = {}
    for route in routes:
        on_route(ctx, route)
        outs[route], r = run.boxed(ctx, flat)
        assert r == route, (M, k, route, r)
        launched(ctx, route)
        feasible = check_against_oracle(outs[route], inst, run, M, k, route)
        assert feasible == sum(pb.answer(f, k, kind)[1] == 0 for f, kind in inst) >= len(inst) // 2, (route, feasible)
    print(f"M = {M} k = {k}: {len(inst)} instances, {feasible} feasible")
    for route in routes[1:]:
        close_outputs(outs[route], outs[routes[0]], (M, k, route))


# ------------------------------------------------------------------ 2. pins against halda_eval_plans
@pytest.mark.parametrize("route,M,k", [("fused", 64, 1), ("tables", 16, 1), ("tables", 16, 2), ("tables", 5, 4),
                                       ("general", 16, 2), ("general", 64, 1)])
def test_pinned_boxes_under_pressure_price_the_plan_as_eval_plans_does(ctx, route, M, k):
    inst, run, flat, table = batch(M, k, ("pin",))
    on_route(ctx, route)
    got, r = run.boxed(ctx, flat)
    assert r == route
    launched(ctx, route)
    w1, n1 = flat[0], flat[2]
    buf = pl.evaluate_table(table, pc.our_model(), np.full(len(inst), k, np.int32), w1, n1, KV)
    feasible = 0
    for i, (f, _) in enumerate(inst):
        assert (got["status"][i] == lh.STATUS_OPTIMAL) == (buf.status[i] == lh.STATUS_OPTIMAL), f
        assert (buf.status[i] == lh.STATUS_OPTIMAL) == (pb.answer(f, k, "pin")[1] == 0), f
        if buf.status[i] != lh.STATUS_OPTIMAL:
            assert got["status"][i] == lh.STATUS_INFEASIBLE and got["best_k"][i] == 0, f
            continue
        feasible += 1
        a = i * M
        assert np.array_equal(got["w"][a:a + M], w1[a:a + M]) and np.array_equal(got["n"][a:a + M], n1[a:a + M]), f
        if route == "general":
            assert abs(got["obj_value"][i] - buf.obj[i]) <= 1e-12 * max(1.0, abs(buf.obj[i])), f
        else:
            assert got["obj_value"][i] == buf.obj[i], f
    assert feasible >= len(inst) // 2


# ------------------------------------------------------------------ 3. an n box that never binds
@pytest.mark.parametrize("route,M,k", [("fused", 64, 1), ("tables", 16, 2), ("tables", 5, 4), ("general", 16, 2)])
def test_a_never_binding_n_box_under_pressure_equals_the_bounded_call(ctx, route, M, k):
    """The D = 2 move box on w around the pressured incumbent, n_min = 0 and n_max = W: every output, x included,
    is halda_solve_fleets_bounded's bit for bit."""
    inst, run, flat, table = batch(M, k, ("box2",), pb.pressured_fleets(M))
    W = L // k
    on_route(ctx, route)
    want, r = run.bounded(ctx, flat[0], flat[1])
    assert r == route
    launched(ctx, route)
    assert (want["best_k"] == k).sum() >= len(inst) // 2
    nd = table.n_devices
    got, r = run.boxed(ctx, (flat[0], flat[1], np.zeros(nd, np.int32), np.full(nd, W, np.int32)))
    assert r == route
    launched(ctx, route)
    same(got, want)
    x = want["x"].reshape(len(inst), -1)[want["best_k"] == k]
    assert (x[:, 2 * M:6 * M] > 0.5).any(axis=1).mean() >= 0.9  # these optima do use their slacks


# ------------------------------------------------------------------ 4. the DP test path
@pytest.mark.parametrize("route,M,k", [("fused", 64, 1), ("tables", 16, 4), ("tables", 5, 1), ("tables", 16, 2)])
def test_dp_path_gives_the_same_answers_on_push_and_tcap_cases(ctx, route, M, k):
    inst, run, flat, _ = batch(M, k, ("push", "tcap", "off"))
    if k != 2:
        assert any(kind == "tcap" for _, kind in inst)
    on_route(ctx, route)
    greedy, r = run.boxed(ctx, flat)
    assert r == route
    ctx.set_fleets_path("dp")
    dp, r = run.boxed(ctx, flat)
    ctx.set_fleets_path("fused")
    assert r == route
    if route == "fused":
        same(dp, greedy)
    else:
        close_outputs(dp, greedy, (route, M, k))
    assert check_against_oracle(dp, inst, run, M, k, f"dp / {route}") >= len(inst) // 3


# ------------------------------------------------------------------ 5. the Python entries
def test_solve_bounded_with_n_max_under_pressure(ctx):
    """n_max_i = 0 on the device with the largest GPU share (the "off" kind) through halda_solve_bounded."""
    model = pc.our_model()
    for f, k, route, ask in ((("p", (64, pc.S64, 0, "4bit")), 1, "fused", "auto"),
                             (("p", (16, pc.S16, 1, "4bit")), 2, "tables", "tables"),
                             (("p", (5, pc.S16, 2, "4bit")), 4, "general", "general")):
        M = f[1][0]
        b, st, x, _, obj, unique = pb.answer(f, k, "off")
        i = int(np.argmin(b[3]))
        assert st == 0 and b[3][i] == 0 and pb.free_optimum(f, k)[2][i] > 0
        r = halda_solve_bounded(pb.devices(f), model, n_max=b[3], k_candidates=[k], kv_bits="4bit", route=ask)
        assert bd.last_bounds_route(ctx) == route, (f, bd.last_bounds_route(ctx))
        assert r.k == k and r.n[i] == 0 and sum(r.w) == L // k
        assert pc.close(r.obj_value, obj), (f, r.obj_value, obj)
        if unique:
            assert r.w + r.n == [int(v) for v in np.rint(x[:2 * M])], f


def test_replace_within_with_an_n_budget_under_pressure(ctx):
    """halda_replace_within(max_move=2, max_move_n=2) around the pressured incumbent (the "box2" kind)."""
    model = pc.our_model()
    for f, k, route, ask in ((("p", (64, pc.S16, 1, "4bit")), 1, "fused", "auto"),
                             (("p", (16, pc.S64, 2, "4bit")), 2, "tables", "tables"),
                             (("p", (16, pc.S16, 3, "4bit")), 4, "tables", "tables")):
        M = f[1][0]
        w1, n1 = pb.incumbent(f, k)
        b, st, x, _, obj, unique = pb.answer(f, k, "box2")
        assert st == 0
        r = halda_replace_within(pb.devices(f), model, (k, list(w1), list(n1)), 2, kv_bits="4bit", route=ask,
                                 max_move_n=2)
        assert bd.last_bounds_route(ctx) == route, (f, bd.last_bounds_route(ctx))
        assert r.within is not None and r.within.k == k and pc.close(r.within.obj_value, obj), (f, r.within, obj)
        assert all(lo <= v <= hi for lo, v, hi in zip(b[0], r.within.w, b[1])), f
        assert all(lo <= v <= hi for lo, v, hi in zip(b[2], r.within.n, b[3])), f
        assert r.moved_layers_within == sum(abs(a - c) for a, c in zip(r.within.w, w1)) <= 2 * M
        assert r.moved_gpu_layers_within == sum(abs(a - c) for a, c in zip(r.within.n, n1)) <= 2 * M
        assert r.gap_to_free >= 0.0 and r.best is not None
        if unique:
            assert r.within.w + r.within.n == [int(v) for v in np.rint(x[:2 * M])], f
