"""The bounded sweep's table route on the GPU (bounds path 3, halda_sweep_bounds_tables_kernel): bounds that never
bind give the table sweep's bits, binding bounds the exact oracle's plans, the table route equals the general one
(and yields to it beyond its gate), the infeasible and edge cases, the DP test path, memory pressure, the Python
entries' `route` keyword, a resident table and two streams. The route is asserted in every case."""

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import halda_solve_batch
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import DeviceFleetTable, fleet_table, solve_table
from oracle import milp_oracle as mo

from . import bounds_cases as bc
from . import pressure_cases as pc
from .test_gpu_bounds import IMAX, KV, Run, _torch, check_against_oracle, fleet, noop_variants, same

pytestmark = pytest.mark.gpu

MIXED = (1, 2, 3, 15, 16, 17, 33, 40)  # over the lane-group and chunk boundaries of table_pass, all <= 64
LDS_BUDGET = 160 * 1024


@pytest.fixture
def ctx():
    c = lh.get_context(0)
    bd.set_bounds_path(c, 3)
    yield c
    c.set_fleets_path("fused")
    c.set_timing(False)
    bd.set_bounds_path(c, 0)


@pytest.fixture(scope="module")
def mixed(llama_online_model):
    return fleet_table([fleet(M, 300 + M) for M in MIXED], llama_online_model)


def binding_boxes(table, model, ks, seed=11):
    """free.w -/+ 0 .. 2 per device around the free optimum over ks (the host-lowering test's boxes)."""
    rng = np.random.default_rng(seed)
    free = solve_table(table, model, ks, KV)
    lo = np.maximum(1, free.w - rng.integers(0, 3, table.n_devices)).astype(np.int32)
    hi = np.minimum(int(model.L), free.w + rng.integers(0, 3, table.n_devices)).astype(np.int32)
    return lo, hi


def close_outputs(a, b, what):
    """Status, best k and plan equal; the objectives with the same finiteness and within the cross-path bound."""
    for f in ("status", "best_k", "w", "n"):
        assert np.array_equal(a[f], b[f]), (what, f)
    for f in ("obj_value", "obj_by_k"):
        x, y = a[f], b[f]
        fin = np.isfinite(y)
        assert np.array_equal(np.isfinite(x), fin), (what, f)
        assert (np.abs(x[fin] - y[fin]) <= 1e-12 * np.maximum(1.0, np.abs(y[fin]))).all(), (what, f)


def slice_bytes(mmax, min_devices, L, ks):
    """The table kernel's LDS slice as the library sizes it for an unbounded batch (plan_sweep, make_slice)."""
    a16 = lambda x: (x + 15) & ~15
    r1_k1 = max([L // k - min_devices + 1 for k in ks if k == 1], default=0)
    r1_kc = max([L // k - min_devices + 1 for k in ks if k != 1], default=0)
    r1max = max(1, r1_k1, r1_kc)
    tab = mmax * r1_k1 + mmax if r1_k1 > 0 else 1
    tab_kc = mmax * r1_kc + mmax if r1_kc > 0 else 0
    o = a16(mmax * 4 * 8)                                 # rows
    o = a16(o + mmax * 4 * 8)                             # cyc
    o = a16(o + mmax * 6 * 8)                             # cost
    o = a16(o + mmax * 4)                                 # cnt
    o = a16(o + mmax * 4)                                 # st0
    o = a16(o + mmax * 4)                                 # st1
    o = a16(o + mmax * 8)                                 # rng
    o = a16(o + mmax * 8)                                 # inc
    o = a16(o + max(tab, tab_kc) * 8)                     # G
    o = a16(o + tab_kc * 8)                               # H
    o = a16(o + ((tab_kc // 2 + 2 * r1max + 2) * 8 if tab_kc > 0 else 0))  # work
    return a16(o + (mmax + 12) * r1max * 2)               # split


# ------------------------------------------------------------------ 1. bounds that never bind
NOOP_SHAPES = {"m16": (16, [1, 2, 4, 5]), "m5": (5, [1, 2, 4]), "m33": (33, [1, 2]), "m2": (2, [1, 40]),
               "m1": (1, [1])}


def noop_check(ctx, table, model, ks, what):
    run = Run(table, model, ks)
    ctx.set_fleets_path("wave")  # one fleet per wave: these batches run halda_sweep_tables_kernel alone
    ctx.set_timing(True)
    want = run.plain(ctx)
    assert set(ctx.last_fleet_ms()) == {"halda_sweep_tables_kernel"}, what
    assert (want["best_k"] > 0).all()
    got, route = run.bounded(ctx, None, None, null_struct=True)
    assert route == "tables", what
    same(got, want)
    for lo, hi in noop_variants(table, model, ks):
        got, route = run.bounded(ctx, lo, hi)
        assert route == "tables", what
        same(got, want)


@pytest.mark.parametrize("shape", sorted(NOOP_SHAPES))
def test_noop_bounds_equal_the_table_sweep(ctx, llama_online_model, shape):
    M, ks = NOOP_SHAPES[shape]
    model = llama_online_model
    noop_check(ctx, fleet_table([fleet(M, 1100 + s) for s in range(5)], model), model, ks, shape)


def test_noop_bounds_equal_the_table_sweep_on_mixed_sizes(ctx, llama_online_model, mixed):
    noop_check(ctx, mixed, llama_online_model, [1, 2, 4], "mixed")


# ------------------------------------------------------------------ 2. binding bounds against the exact oracle
PAIRS = [(4, 2), (8, 4), (16, 1), (16, 2), (16, 4), (16, 5), (5, 2), (3, 1), (2, 2), (20, 2), (32, 2), (33, 2),
         (40, 1), (40, 2)]


@pytest.mark.parametrize("M,k", PAIRS)
def test_binding_bounds_on_the_table_route_equal_the_oracle(ctx, llama_online_model, M, k):
    # (40, 1) alone: L - M + 1 = 41 <= 64 at k = 1, so path 3 keeps the register launch (route 1) there
    differ, total = check_against_oracle(ctx, llama_online_model, M, k, "fused" if (M, k) == (40, 1) else "tables")
    print(f"M = {M} k = {k}: {differ} of {total} plans differ from the unbounded optimum")
    assert total == 36
    if (M, k) not in ((16, 5), (40, 2)):  # W = M there: the plan is forced
        assert differ >= 18


def test_path_3_keeps_the_fused_route_where_it_applies(ctx, llama_online_model):
    differ, total = check_against_oracle(ctx, llama_online_model, 64, 1, "fused")
    assert total == 36 and differ >= 24


# ------------------------------------------------------------------ 3. table route equals general route
@pytest.mark.parametrize("ks", [[1, 2, 4], [5, 8]])
def test_table_route_equals_the_general_route(ctx, llama_online_model, mixed, ks):
    model = llama_online_model
    lo, hi = binding_boxes(mixed, model, ks)
    run = Run(mixed, model, ks)
    tab, route = run.bounded(ctx, lo, hi)
    assert route == "tables"
    bd.set_bounds_path(ctx, 1)
    gen, route = run.bounded(ctx, lo, hi)
    assert route == "general"
    close_outputs(tab, gen, ks)
    assert (tab["best_k"] > 0).sum() >= len(MIXED) // 2  # the boxes hold plans


def test_a_slice_beyond_the_lds_budget_goes_general(ctx, llama_online_model):
    """Few-device fleets on a long copy of the model: the unbounded slice (mostly (M + 12) (L - M + 1) split
    entries and the G / H / work tables) exceeds the budget, so path 3 takes the general route."""
    L, ks, sizes = 2400, [1, 2], (2, 3, 3)
    assert slice_bytes(max(sizes), min(sizes), L, ks) > LDS_BUDGET
    assert slice_bytes(max(MIXED), min(MIXED), 80, [1, 2, 4]) <= LDS_BUDGET  # the shapes above do fit
    model = llama_online_model.model_copy(update={"L": L})
    table = fleet_table([fleet(M, 1800 + i) for i, M in enumerate(sizes)], model)
    lo, hi = binding_boxes(table, model, ks)
    run = Run(table, model, ks)
    got, route = run.bounded(ctx, lo, hi)
    assert route == "general"
    bd.set_bounds_path(ctx, 1)
    want, route = run.bounded(ctx, lo, hi)
    assert route == "general"
    same(got, want)
    assert (got["best_k"] > 0).any()


def test_a_65_device_fleet_goes_general(ctx, llama_online_model):
    model = llama_online_model
    table = fleet_table([fleet(M, 1900 + M) for M in (16, 65, 8)], model)
    ks = [1, 2]
    lo, hi = binding_boxes(table, model, ks)
    run = Run(table, model, ks)
    got, route = run.bounded(ctx, lo, hi)
    assert route == "general"
    bd.set_bounds_path(ctx, 1)
    want, route = run.bounded(ctx, lo, hi)
    assert route == "general"
    same(got, want)


# ------------------------------------------------------------------ 4. infeasible and edge cases
def test_infeasible_and_edge_cases(ctx, llama_online_model):
    model = llama_online_model
    M, ks, nf = 16, [1, 2, 4, 5], 7
    devs = [fleet(M, 1300 + s) for s in range(nf)]
    table = fleet_table(devs, model)
    run = Run(table, model, ks)
    w2 = solve_table(table, model, [2], KV).w.reshape(nf, M)  # the free k = 2 optimum
    lo, hi = np.ones((nf, M), np.int32), np.full((nf, M), IMAX, np.int32)
    hi[0, :] = 0                         # fleet 0: sum hi = 0 < W for every k
    lo[1, :] = 6                         # fleet 1: sum lo = 96 > W for every k
    lo[2, 5], hi[2, 5] = 4, 3            # fleet 2: one device with lo > hi
    lo[3, :8], lo[3, 8:] = 3, 2          # fleet 3: sum lo = 40: forced at k = 2 (R = 0, k > 1)
    lo[4, :] = hi[4, :] = w2[4]          # fleet 4: every device pinned at the free k = 2 optimum
    lo[5, 7] = hi[5, 7] = w2[5, 7] + 2   # fleet 5: one device pinned two layers above its k = 2 optimum
    # fleet 6: no bounds
    got, route = run.bounded(ctx, lo.ravel(), hi.ravel())
    assert route == "tables"
    bd.set_bounds_path(ctx, 1)
    gen, route = run.bounded(ctx, lo.ravel(), hi.ravel())
    assert route == "general"
    assert np.array_equal(got["status"], gen["status"])  # per (fleet, k), exactly
    close_outputs(got, gen, "edge")
    st = got["status"].reshape(nf, len(ks))
    assert (st[:3] == lh.STATUS_INFEASIBLE).all() and (got["best_k"][:3] == 0).all()
    assert (got["obj_value"][:3] == np.inf).all() and (got["w"].reshape(nf, M)[:3] == 0).all()
    assert st[3, 1] == lh.STATUS_OPTIMAL and (st[3, 2:] == lh.STATUS_INFEASIBLE).all()
    assert st[4].tolist() == [lh.STATUS_INFEASIBLE, lh.STATUS_OPTIMAL, lh.STATUS_INFEASIBLE, lh.STATUS_INFEASIBLE]
    assert got["best_k"][4] == 2 and np.array_equal(got["w"].reshape(nf, M)[4], w2[4])
    assert st[5, 1] == lh.STATUS_OPTIMAL and st[6, 1] == lh.STATUS_OPTIMAL
    # the forced and the pinned fleets at k = 2 against the exact oracle
    N, j = 7 * M + 1, 1
    for f in (3, 4, 5):
        s_, ow, on, cx, obj, unique = bc.exact_answer(model, devs[f], 2, lo[f].tolist(),
                                                      np.minimum(hi[f], 40).tolist())
        assert s_ == 0, f
        q = f * len(ks) + j
        x, c = got["x"][q * run.xs:q * run.xs + N], got["c"][q * run.xs:q * run.xs + N]
        assert bc.rel(got["obj_by_k"][q], obj) <= 1e-9 and bc.rel(float(c.dot(x)), cx) <= 1e-9, f
        if f in (3, 4) or unique:  # w is forced on fleets 3 and 4
            assert x[:M].tolist() == ow, f
        if unique:
            assert x[M:2 * M].tolist() == on, f
    # every returned (k, w, n) priced by halda_eval_plans
    buf = pl.evaluate_table(table, model, got["best_k"], got["w"], got["n"], KV)
    for f in range(3, nf):
        assert got["best_k"][f] > 0 and buf.status[f] == lh.STATUS_OPTIMAL, f
        assert bc.rel(buf.obj[f], got["obj_value"][f]) <= 1e-12, f


# ------------------------------------------------------------------ 5. the DP test path
@pytest.mark.parametrize("ks", [[1, 2, 4], [5, 8]])
def test_dp_path_under_the_table_route(ctx, llama_online_model, mixed, ks):
    model = llama_online_model
    lo, hi = binding_boxes(mixed, model, ks)
    run = Run(mixed, model, ks)
    greedy, route = run.bounded(ctx, lo, hi)
    assert route == "tables"
    ctx.set_fleets_path("dp")
    dp, route = run.bounded(ctx, lo, hi)
    ctx.set_fleets_path("fused")
    assert route == "tables"
    close_outputs(dp, greedy, ks)


# ------------------------------------------------------------------ 6. memory pressure
@pytest.mark.parametrize("k", [1, 2, 4])
def test_bounded_sweep_under_pressure_on_the_table_route(k):
    """test_gpu_pressure's bounded case with route="tables": the pressured 16-device fleets within the D = 2
    box around the pressured optimum of seed + 100 and within the uniform cap, each against the exact oracle."""
    c = lh.get_context(0)
    model = pc.our_model()
    M, W = 16, pc.L // k
    fleets, boxes, kinds = [], [], []
    for case in pc.cases(Ms=(M,), kvs=("4bit",), seeds=None):
        st, x0, _, _ = pc.exact((M, case[1], case[2] + 100, "4bit"), k)
        assert st == 0
        w0 = [int(v) for v in x0[:M]]
        for kind, box in ((2, ([max(1, v - 2) for v in w0], [min(W, v + 2) for v in w0])),
                          ("cap", ([1] * M, [min(W, -(-W // M) + 1)] * M))):
            fleets.append(pc.devices(case[2], case[0], case[1]))
            boxes.append(box)
            kinds.append((case, kind))
    assert len(fleets) <= 64
    got = bd.halda_solve_bounded_batch(fleets, model, boxes, k_candidates=[k], kv_bits="4bit", route="tables")
    assert bd.last_bounds_route(c) == "tables"
    feasible = 0
    for (case, kind), (lo, hi), r in zip(kinds, boxes, got):
        p = dict(pc.problem(case, k))
        p["lb"], p["ub"] = p["lb"].copy(), p["ub"].copy()
        p["lb"][:M], p["ub"][:M] = lo, hi
        st, xo, b1, b2, _ = mo.exact_solve(p)
        if st != 0:
            assert st == 2 and r is None, (case, kind, r)  # an empty box comes back None
            continue
        feasible += 1
        assert r is not None and r.k == k, (case, kind)
        assert pc.close(r.obj_value, mo.objective_value(p, xo)), (case, kind, r.obj_value)
        assert all(a <= v <= b for a, v, b in zip(lo, r.w, hi)), (case, kind)
        if mo.uniqueness_margin_ok(b1, b2):
            assert r.w == [int(v) for v in xo[:M]] and r.n == [int(v) for v in xo[M:2 * M]], (case, kind, r)
    print(f"bounded M = {M} k = {k}: {feasible} of {len(got)} feasible")
    assert feasible >= 0.5 * len(got), (feasible, len(got))


# ------------------------------------------------------------------ 7. the Python entries
def result_key(r):
    return None if r is None else (r.k, r.w, r.n, r.obj_value, r.sets)


def test_bounded_batch_route_keyword(llama_online_model):
    c = lh.get_context(0)
    model = llama_online_model
    fleets = [fleet(M, 1600 + M) for M in (3, 8, 8, 20)]
    ks = [1, 2, 10]
    free1 = halda_solve_batch(fleets[1:2], model, k_candidates=[2], kv_bits="4bit")[0]
    i = int(np.argmax(free1.w))  # fleet 1: its largest k = 2 share capped one layer lower
    hi1 = [80] * 8
    hi1[i] = free1.w[i] - 1
    cap = [None, ([1] * 8, hi1), ([2] * 8, [6] * 8), ([1] * 20, [5] * 20)]
    bd.set_bounds_path(c, 0)
    try:
        tab = bd.halda_solve_bounded_batch(fleets, model, cap, k_candidates=ks, kv_bits="4bit", route="tables")
        assert bd.last_bounds_route(c) == "tables"
        gen = bd.halda_solve_bounded_batch(fleets, model, cap, k_candidates=ks, kv_bits="4bit", route="general")
        assert bd.last_bounds_route(c) == "general"
        assert all(r is not None for r in tab)
        assert [result_key(r) for r in tab] == [result_key(r) for r in gen]
        # the context's path is back at 0: the automatic route of this shape is the general one
        auto = bd.halda_solve_bounded_batch(fleets, model, cap, k_candidates=ks, kv_bits="4bit")
        assert bd.last_bounds_route(c) == "general"
        assert [result_key(r) for r in auto] == [result_key(r) for r in gen]
        # and a path set on the context survives a call that overrides it
        bd.set_bounds_path(c, 3)
        bd.halda_solve_bounded_batch(fleets, model, cap, k_candidates=ks, kv_bits="4bit", route="general")
        assert bd.last_bounds_route(c) == "general"
        auto3 = bd.halda_solve_bounded_batch(fleets, model, cap, k_candidates=ks, kv_bits="4bit")
        assert bd.last_bounds_route(c) == "tables"
        assert [result_key(r) for r in auto3] == [result_key(r) for r in tab]
    finally:
        bd.set_bounds_path(c, 0)


@pytest.mark.parametrize("M", [8, 16])
def test_replace_within_on_the_table_route(llama_online_model, M):
    c = lh.get_context(0)
    model = llama_online_model
    devs = fleet(M, 1400 + M)
    inc = halda_solve_batch([fleet(M, 1500 + M)], model, k_candidates=[2], kv_bits="4bit")[0]
    assert inc.k == 2
    for D in (1, 2):
        r = bd.halda_replace_within(devs, model, inc, D, kv_bits="4bit", route="tables")
        assert bd.last_bounds_route(c) == "tables"
        g = bd.halda_replace_within(devs, model, inc, D, kv_bits="4bit", route="general")
        assert bd.last_bounds_route(c) == "general"
        lo, hi = bd.move_bounds(inc.w, D)
        assert r.within is not None and r.within.k == 2
        assert all(l <= v <= h for l, v, h in zip(lo, r.within.w, hi)) and sum(r.within.w) == model.L // 2
        assert r.moved_layers_within == sum(abs(a - b) for a, b in zip(r.within.w, inc.w)) <= D * M
        assert result_key(r.within) == result_key(g.within)
        assert r.moved_layers_within == g.moved_layers_within and r.gap_to_free >= 0.0
        # the context's path is back at its previous value (0: this shape's automatic route is the general one)
        bd.halda_solve_bounded_batch([devs], model, [(lo, hi)], k_candidates=[2], kv_bits="4bit")
        assert bd.last_bounds_route(c) == "general"


# ------------------------------------------------------------------ 8. a resident table
def test_resident_bounds_follow_their_contents(ctx, llama_online_model):
    torch, dev = _torch()
    model = llama_online_model
    M, nf = 16, 6
    table = fleet_table([fleet(M, 1700 + s) for s in range(nf)], model)
    dt = DeviceFleetTable(table, model, [1, 2, 4, 5], KV, dev)
    dt.set_bounds()
    s = torch.cuda.Stream(dev)
    dt.launch_with_bounds(ctx, s.cuda_stream)
    torch.cuda.synchronize(dev)
    assert bd.last_bounds_route(ctx) == "tables"
    out0 = {f: dt.out[f].cpu().numpy().copy() for f in ("best_k", "obj_value", "w", "n")}
    w0, best = out0["w"], out0["obj_value"]
    assert (out0["best_k"] > 0).all()
    d1 = M + int(np.argmax(w0[M:2 * M]))  # fleet 1's device with the most layers
    assert w0[d1] > 1
    with torch.cuda.stream(s):  # in place: fleet 0 pinned at its optimum, one device of fleet 1 one layer lower
        dt.bound_min[:M].copy_(dt.out["w"][:M])
        dt.bound_max[:M].copy_(dt.out["w"][:M])
        dt.bound_max[d1] = int(w0[d1]) - 1
    dt.launch_with_bounds(ctx, s.cuda_stream)
    torch.cuda.synchronize(dev)
    assert bd.last_bounds_route(ctx) == "tables"
    out1 = {f: dt.out[f].cpu().numpy() for f in ("best_k", "obj_value", "w", "n")}
    assert np.array_equal(out1["w"][:M], w0[:M]) and out1["best_k"][0] == out0["best_k"][0]
    assert bc.rel(out1["obj_value"][0], best[0]) <= 1e-12  # the same plan, at R = 0 by the register greedy
    assert out1["w"][d1] <= w0[d1] - 1 and out1["obj_value"][1] >= best[1]
    for f in ("w", "n"):
        assert np.array_equal(out1[f][2 * M:], out0[f][2 * M:]), f
    for f in ("best_k", "obj_value"):
        assert np.array_equal(out1[f][2:], out0[f][2:]), f  # the untouched fleets keep their bits


# ------------------------------------------------------------------ 9. two streams
def test_launches_on_two_streams_keep_their_own_outputs(ctx, llama_online_model):
    torch, dev = _torch()
    model = llama_online_model
    ks = [1, 2, 4, 5]
    tabs, want = [], []
    for t in range(2):
        table = fleet_table([fleet(16, 2000 + 10 * t + s) for s in range(6)], model)
        lo, hi = binding_boxes(table, model, ks, seed=20 + t)
        dt = DeviceFleetTable(table, model, ks, KV, dev, want_per_k=True)
        dt.set_bounds(lo, hi)
        dt.launch_with_bounds(ctx, 0)  # the synchronous call's outputs
        torch.cuda.synchronize(dev)
        assert bd.last_bounds_route(ctx) == "tables"
        want.append({f: v.cpu().numpy().copy() for f, v in dt.out.items()})
        tabs.append(dt)
    assert not np.array_equal(want[0]["w"], want[1]["w"])
    for dt in tabs:
        for v in dt.out.values():
            v.fill_(-7)
    torch.cuda.synchronize(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for _ in range(3):
        for dt, s in zip(tabs, streams):
            dt.launch_with_bounds(ctx, s.cuda_stream)
            assert bd.last_bounds_route(ctx) == "tables"
    torch.cuda.synchronize(dev)
    for dt, w in zip(tabs, want):
        for f, v in dt.out.items():
            assert np.array_equal(v.cpu().numpy(), w[f], equal_nan=True), f
