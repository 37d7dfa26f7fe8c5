"""Homogeneous and duplicated fleets (tests/tied_cases.py) on every GPU route, each against the exact oracle.

On these fleets the optimum is almost never unique, so the documented tie rules decide which plan comes back and the
usual column-by-column comparison is idle. Every route's (w, n) is therefore re-priced by the oracle with both column
groups pinned (tied_cases.check_plan): the plan must be feasible and price at the oracle's optimum within 1e-9, the
route's reported objective likewise, and (w, n) equal the oracle's wherever the optimum is unique. Contracts that
promise bits (sub-fleets, variants, plans, boxes, change against budget, subsets and scale against their per-list
entries) are held to bits on tied parents, and the tie rules that name an index (the first d droppable devices, the
last a pool devices, the lowest bottleneck index) are asserted where every candidate ties."""

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import halda_solve_batch
from distilp_amd.solver import plans as pl
from distilp_amd.solver.batch import assemble, settled_instances
from distilp_amd.solver.fleets import DeviceFleetTable, PlanGroup, fleet_table, solve_table
from distilp_amd.solver.lower import lower_fleet

from . import tied_cases as tc

pytestmark = pytest.mark.gpu

OUTS = ("best_k", "obj_value", "w", "n", "obj_by_k", "status")
CSR_KERNELS = {"halda_lower_kernel", "halda_screen_kernel", "halda_solve_k1_kernel", "halda_solve_kernel"}


@pytest.fixture(scope="module")
def ctx():
    c = lh.get_context(0)
    yield c
    c.set_fleets_path("fused")
    c.set_timing(False)
    pl.set_plans_path(c, 0)


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


def class_of(cases):
    """The (M, L) class whose model and k list a batch runs on: all of one L."""
    assert len({tc.L_of(c) for c in cases}) == 1
    return cases[0][0]


_SWEEPS = {}


def sweep(ctx, name, cases, path="fused", fresh=False):
    """solve_table(want_x=True) of the cases' fleets over the class's k list on a fleets path, and the kernels that
    ran. Kept per (name, path): the sweeps are shared among the tests, read only."""
    key = (name, path)
    if fresh or key not in _SWEEPS:
        model = tc.model_of(cases[0])
        table = fleet_table([tc.devices(c) for c in cases], model)
        ctx.set_fleets_path(path)
        ctx.set_timing(True)
        try:
            res = solve_table(table, model, tc.sweep_ks(class_of(cases)), tc.KV, want_x=True)
            ran = set(ctx.last_fleet_ms())
        finally:
            ctx.set_fleets_path("fused")
            ctx.set_timing(False)
        if fresh:
            return table, res, ran
        _SWEEPS[key] = (table, res, ran)
    return _SWEEPS[key]


def check_sweep(cases, table, res, what):
    """A FleetSolve (dense x) against the oracle: per (fleet, k) the status and check_plan on x's w / n columns; per
    fleet the best k by the reference's strict "<" (skipped where the two best are within 1e-7), obj_value, (w, n)."""
    ks = tc.sweep_ks(class_of(cases))
    for f, case in enumerate(cases):
        M, L = tc.M_of(case), tc.L_of(case)
        a = int(table.dev_off[f])
        best = None
        for j, k in enumerate(ks):
            if L // k < M or tc.exact(case, k)[0] != 0:
                assert L // k < M or tc.exact(case, k)[0] == 2, (what, case, k)
                assert res.status[f, j] == lh.STATUS_INFEASIBLE and np.isinf(res.obj_by_k[f, j]), (what, case, k)
                continue
            assert res.status[f, j] == lh.STATUS_OPTIMAL, (what, case, k, res.status[f, j])
            x = res.x[f, j, :7 * M + 1]
            tc.check_x(case, k, x, res.obj_by_k[f, j], what)
            obj = float(res.obj_by_k[f, j])
            if best is None or obj < best[0]:
                best = (obj, k, x)
        assert best is not None and res.best_k[f] == best[1], (what, case, int(res.best_k[f]), best[1])
        assert tc.close(float(res.obj_value[f]), best[0]), (what, case)
        assert np.array_equal(res.w[a:a + M], best[2][:M]) and np.array_equal(res.n[a:a + M], best[2][M:2 * M]), (
            what, case)
        tc.check_plan(case, best[1], res.w[a:a + M], res.n[a:a + M], res.obj_value[f], what)
        if tc.best_k_decided(case, ks):
            assert res.best_k[f] == tc.best_k(case, ks)[0], (what, case, int(res.best_k[f]), tc.best_k(case, ks))


BATCHES = {
    "T64": (lambda: tc.cases("T64"), {"fused": {"halda_sweep_kernel"}}),
    "T33": (lambda: tc.cases("T33"), {}),
    "T16p": (tc.kslot_batch, {"fused": {"halda_sweep_kslot_kernel"}, "kslot_unsplit": {"halda_sweep_kslot_kernel"},
                              "kslot_sequential": {"halda_sweep_kslot_kernel"}, "seg": {"halda_sweep_seg_kernel"}}),
    "T70": (lambda: tc.cases("T70"), {}),
    "D64": (lambda: tc.cases("D64"), {}),
    "mixed": (tc.mixed_batch, {}),
}
PATHS = ("fused", "dp", "wave", "csr")


def paths_of(name):
    return PATHS + (("seg", "kslot_unsplit", "kslot_sequential") if name == "T16p" else ())


@pytest.mark.parametrize("name", list(BATCHES))
def test_every_fleets_path_returns_an_optimal_plan(ctx, name):
    """solve_table on each halda_set_fleets_path path: every optimal (fleet, k) through check_plan, the statuses,
    best k, obj_value and the result's (w, n); status and best k equal among the paths. A plan that differs between
    two paths of a tied instance is no defect (the greedy and the DP break ties differently): they are counted."""
    make, kernels = BATCHES[name]
    cases = make()
    runs, dev_off = {}, None
    for path in paths_of(name):
        table, res, ran = sweep(ctx, name, cases, path)
        if dev_off is None:
            dev_off = table.dev_off.copy()
        assert np.array_equal(table.dev_off, dev_off), path  # every path packs the same table
        print(f"{name} / {path}: {len(cases)} fleets, kernels {sorted(ran)}")
        assert ran, path
        if path == "csr":
            assert "halda_lower_kernel" in ran, ran
        else:
            assert not (ran & CSR_KERNELS), (path, ran)
        if path in kernels:
            assert kernels[path] <= ran, (name, path, ran)
        if name == "T64" and path == "fused":
            assert ran == {"halda_sweep_kernel"}, ran
        check_sweep(cases, table, res, f"{name} / {path}")
        runs[path] = res
    differ = set()
    for path, res in runs.items():
        assert np.array_equal(res.status, runs["fused"].status), (name, path)
        assert np.array_equal(res.best_k, runs["fused"].best_k), (name, path)
        for f in range(len(cases)):
            a, b = int(dev_off[f]), int(dev_off[f + 1])
            ref = runs["fused"]
            if not (np.array_equal(res.w[a:b], ref.w[a:b]) and np.array_equal(res.n[a:b], ref.n[a:b])):
                differ.add(cases[f])
    print(f"{name}: {len(differ)} of {len(set(cases))} distinct fleets return another optimal (w, n) on another path")


@pytest.mark.parametrize("name", ["T64", "T33"])
def test_sweeps_are_deterministic(ctx, name):
    cases = BATCHES[name][0]()
    a = sweep(ctx, name, cases)[1]
    b = sweep(ctx, name, cases, fresh=True)[1]
    for f in OUTS + ("x", "c"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (name, f)


# ------------------------------------------------------------------ the CSR pipeline on host-lowered batches
@pytest.mark.parametrize("cls", ["T64", "T33", "T16p"])
def test_csr_pipeline_on_host_lowered_batches(ctx, cls):
    """get_context(0).solve(assemble([lower_fleet(...)])) and the same batch with the settled flags
    (tests/test_gpu_settled.py's _device_solve): check_plan per instance."""
    torch, dev = _torch()

    from .test_gpu_settled import _device_solve

    cases = tc.cases(cls)
    model = tc.model_of(cases[0])
    ks = tc.sweep_ks(cls)
    lowered = [lower_fleet(tc.devices(c), model, tc.KV_BITS) for c in cases]
    b, refs = assemble(lowered, [ks] * len(lowered))
    res = ctx.solve(b)
    settled = _device_solve(ctx, b, settled_instances(b), dev, torch.cuda.Stream(dev))
    solved = 0
    for idx, ref in enumerate(refs):
        case, k = cases[ref.fleet], ref.k
        room = tc.L_of(case) // k >= tc.M_of(case)
        for what, status, xs, obj_lin in (("solve", res.status, res.x, res.obj_lin),
                                          ("settled", settled["status"], settled["x"], settled["obj_lin"])):
            if not room:
                assert status[idx] == lh.STATUS_INFEASIBLE, (what, case, k)
                continue
            assert status[idx] == lh.STATUS_OPTIMAL, (what, case, k, int(status[idx]))
            assert tc.close(float(obj_lin[idx]), tc.exact(case, k)[2]), (what, case, k)
            x = np.asarray(xs[ref.col_off:ref.col_off + ref.n_cols], np.float64)
            tc.check_x(case, k, x, tc.mo.objective_value(tc.problem(case, k), x), what)
            solved += 1
    assert solved == 2 * len(tc.instances(cases))


# ------------------------------------------------------------------ steps / group launch
def check_resident(ctx, name, cases, table, dt, what):
    """A resident table's outputs: check_plan at its best k, and every output bit for bit its own solve_table's."""
    out = {k: v.cpu().numpy() for k, v in dt.out.items()}
    _, res, _ = sweep(ctx, name, cases)
    for f in OUTS:
        assert out[f].tobytes() == np.ascontiguousarray(getattr(res, f)).tobytes(), (what, f)
    for f, case in enumerate(cases):
        a, M = int(table.dev_off[f]), tc.M_of(case)
        kb = int(out["best_k"][f])
        assert kb > 0, (what, case)
        tc.check_plan(case, kb, out["w"][a:a + M], out["n"][a:a + M], out["obj_value"][f], what)
        if tc.best_k_decided(case, tc.sweep_ks(case[0])):
            assert kb == tc.best_k(case)[0], (what, case, kb)


def group_run(ctx, sets, names):
    torch, dev = _torch()
    stream = torch.cuda.Stream(dev)
    tabs = []
    for cs in sets:
        model = tc.model_of(cs[0])
        table = fleet_table([tc.devices(c) for c in cs], model)
        tabs.append((table, DeviceFleetTable(table, model, tc.sweep_ks(cs[0][0]), tc.KV, dev, want_per_k=True)))
    group = PlanGroup([dt for _, dt in tabs], ctx)
    try:
        assert group.persistent
        for _, dt in tabs:
            for v in dt.out.values():
                v.zero_()
        torch.cuda.synchronize(dev)
        ctx.set_timing(True)
        try:
            group.launch(1, 7, stream.cuda_stream)
            torch.cuda.synchronize(dev)
            ran = set(ctx.last_fleet_ms())
        finally:
            ctx.set_timing(False)
        for name, cs, (table, dt) in zip(names, sets, tabs):
            check_resident(ctx, name, cs, table, dt, f"group {name}")
    finally:
        group.close()
    return ran


def test_steps_launch_rotates_three_tied_tables(ctx):
    """Three resident T64 tables (the six fleets of memory scale 1, of 1/16 and of 1/64) rotated over 7 steps from
    first = 1 in one launch of the steps kernel, the outputs zeroed first."""
    sets = [tc.cases("T64", scales=(sc,)) for sc in (tc.S1, tc.S16, tc.S64)]
    assert all(len(cs) == 6 for cs in sets)
    ran = group_run(ctx, sets, [f"T64@{sc}" for sc in (tc.S1, tc.S16, tc.S64)])
    print(f"steps launch T64: kernels {sorted(ran)}")
    assert ran and "halda_sweep_kslot_kernel" not in ran and not (ran & CSR_KERNELS), ran


def test_kslot_group_launch_on_two_tied_tables(ctx):
    sets = [tc.cases("T16p", scales=(sc,)) * 11 for sc in (tc.S16, tc.S64)]
    assert all(len(cs) > 64 for cs in sets)
    ran = group_run(ctx, sets, [f"T16p@{sc}x11" for sc in (tc.S16, tc.S64)])
    print(f"k-slot group launch T16p: kernels {sorted(ran)}")
    assert "halda_sweep_kslot_kernel" in ran, ran


# ------------------------------------------------------------------ sub-fleets
def test_leave_one_out_on_tied_parents(ctx):
    """halda_leave_one_out_batch on one T64 copies fleet and one T64 half fleet (scale 1/64), on the fused route and
    on the expansion path: each equals halda_solve_batch of the materialised lists (pydantic ==); on copies every
    list is the same 63 devices, so all M rows are equal, obj_value bit for bit."""
    from distilp_amd.solver import subfleets as sf

    parents = [tc.cases("T64", kinds=(kind,), scales=(tc.S64,), seeds=(21000,))[0] for kind in ("copies", "half")]
    fleets = [tc.devices(c) for c in parents]
    model = tc.model(80)
    wants = [halda_solve_batch([devs[:i] + devs[i + 1:] for i in range(64)], model, kv_bits=tc.KV_BITS)
             for devs in fleets]
    try:
        for path, route in ((0, "fused"), (1, "expand")):
            sf.set_subfleets_path(ctx, path)
            got = sf.halda_leave_one_out_batch(fleets, model, kv_bits=tc.KV_BITS)
            print(f"leave-one-out path {path}: route {sf.last_subfleets_route(ctx)}")
            assert sf.last_subfleets_route(ctx) == route, (path, sf.last_subfleets_route(ctx))
            for case, row, want in zip(parents, got, wants):
                assert row == want, (path, case)
                assert all(r is not None for r in row), (path, case)
                if case[1] == "copies":
                    assert all(r == row[0] and r.obj_value == row[0].obj_value for r in row), (path, case)
    finally:
        sf.set_subfleets_path(ctx, 0)


# ------------------------------------------------------------------ variants
@pytest.mark.parametrize("name", ["T64", "T33"])
def test_variants_on_tied_fleets(name):
    """halda_solve_variants over kv 4bit / 8bit / fp16 equals one halda_solve_fleets call per variant bit for bit,
    fused and looped (tests/test_gpu_variants.py's check_variants, which asserts the route)."""
    from .test_gpu_variants import check_variants

    model = tc.model(80)
    cases = tc.cases("T64") if name == "T64" else tc.cases("T33", kinds=("half",), scales=(tc.S16,), seeds=(21000,))
    variants = [(model, "4bit"), (model, "8bit"), (model, "fp16")]
    wants = check_variants([tc.devices(c) for c in cases], variants, ks=tc.sweep_ks(name),
                           paths=((0, "fused"), (1, "loop")))
    assert (wants[0]["best_k"] > 0).all()


# ------------------------------------------------------------------ plans
@pytest.mark.parametrize("path", [0, 2])
def test_sweep_with_incumbents_on_tied_fleets(ctx, path):
    """halda_solve_fleets_plans on plan path 0 and plan path 2 on the T64 batch, the incumbent the rolled optimum: the
    sweep through check_plan, the incumbent's evaluation against evaluate_plan_np, and the sweep's own (best_k, w, n)
    evaluates to its obj_value bit for bit against the one-fleet-per-wave sweep."""
    cases = tc.cases("T64")
    model = tc.model(80)
    ks = tc.sweep_ks("T64")
    table = fleet_table([tc.devices(c) for c in cases], model)
    inc = [(1, tc.rolled_w0(c, 1), list(np.roll(tc.plan_of(c, 1)[1], tc.roll_of(c)))) for c in cases]
    k, w, n = pl._plan_arrays(table, inc, allow_none=False)
    pl.set_plans_path(ctx, path)
    try:
        res, buf = pl.solve_plans_table(table, model, ks, k, w, n, tc.KV)
        route = pl.last_plans_route(ctx)
    finally:
        pl.set_plans_path(ctx, 0)
    print(f"plans path {path}: route {route}")
    assert route == ("two_launch" if path == 0 else "fused"), route
    for f, case in enumerate(cases):
        a, M = int(table.dev_off[f]), 64
        e = pl.evaluate_plan_np(table, model, f, *inc[f], tc.KV)
        assert (buf.status[f], buf.reason[f], buf.bottleneck[f]) == (e.status, e.reason, e.bottleneck), (case, e)
        if e.feasible:
            assert buf.cycle[f] == e.cycle and tc.close(float(buf.obj[f]), e.obj_value), case
            got = tc.pinned_price(case, 1, inc[f][1], inc[f][2])
            assert got is not None and tc.close(e.obj_value, got), (case, e.obj_value, got)
        assert res.best_k[f] == 1 and res.status[f, 0] == lh.STATUS_OPTIMAL, case
        tc.check_plan(case, 1, res.w[a:a + M], res.n[a:a + M], res.obj_value[f], f"plans path {path}")
    wave = sweep(ctx, "T64", cases, "wave")[1]
    own = pl.evaluate_table(table, model, wave.best_k, wave.w, wave.n, tc.KV)
    assert (own.status == lh.STATUS_OPTIMAL).all() and (own.reason == 0).all()
    assert np.array_equal(own.obj, wave.obj_value)  # bit for bit
    assert np.array_equal(wave.best_k, res.best_k)
    assert np.allclose(own.obj, res.obj_value, rtol=1e-12, atol=0.0)


def test_plan_evaluation_on_tied_optima_and_neighbours():
    """halda_evaluate_plans_batch on each T64 / T33 / T16p oracle optimum and its six neighbours: status, reason,
    bottleneck and cycle of evaluate_plan_np (tests/test_gpu_plans.py's _check_against_np); on copies fleets the
    GPU's bottleneck is the lowest index holding its (w, n) pair."""
    from distilp_amd.solver import halda_evaluate_plans_batch

    from .test_gpu_plans import _check_against_np

    model = tc.model(80)
    rng = np.random.default_rng(tc.pc.NEIGHBOUR_SEED)
    tabs, plans = {}, []
    for case, k in tc.instances(tc.cases("T64") + tc.cases("T33") + tc.cases("T16p")):
        if case not in tabs:
            tabs[case] = fleet_table([tc.devices(case)], model)
        w, n = tc.plan_of(case, k)
        plans.append((case, tc.devices(case), k, w, n, True, tc.objective(case, k)))
        for _, w2, n2 in tc.pc.neighbours(rng, w, n):
            e = pl.evaluate_plan_np(tabs[case], model, 0, k, w2, n2, tc.KV)
            plans.append((case, tc.devices(case), k, w2, n2, e.feasible, e.obj_value))
    _check_against_np(plans, model)
    copies = [p for p in plans if p[0][1] == "copies"]
    evs = halda_evaluate_plans_batch([p[1] for p in copies], model, [(p[2], p[3], p[4]) for p in copies], tc.KV_BITS)
    seen = 0
    for (case, _, k, w, n, ok, _), e in zip(copies, evs):
        if ok:
            b = e.bottleneck
            assert b == min(i for i in range(len(w)) if (w[i], n[i]) == (w[b], n[b])), (case, k, b, w, n)
            seen += 1
    assert seen >= len(tc.instances(tc.cases("T64", kinds=("copies",))))


# ------------------------------------------------------------------ sharded sweep
@pytest.mark.parametrize("world", [2, 3, 10])
def test_sharded_sweep_on_the_mixed_tied_batch(ctx, world):
    """launch_sharded_emulated on the mixed tied batch: every virtual rank ends with the single-GPU sweep's outputs;
    on the T64 fleets with ks = [2, 4] no k has room: best_k 0, obj_value +inf, w / n as the single-GPU sweep's."""
    from distilp_amd.solver.fleets import launch_sharded_emulated

    torch, dev = _torch()
    stream = torch.cuda.Stream(dev)
    model = tc.model(80)
    for cases, ks in ((tc.mixed_batch(), tc.sweep_ks("T64")), (tc.cases("T64"), [2, 4])):
        table = fleet_table([tc.devices(c) for c in cases], model)
        a = DeviceFleetTable(table, model, ks, tc.KV, dev, want_per_k=True)
        a.launch(ctx, stream.cuda_stream)
        for rank in sorted({0, world // 2, world - 1}):
            b = DeviceFleetTable(table, model, ks, tc.KV, dev, want_per_k=True)
            for t in b.out.values():
                t.fill_(-7)
            launch_sharded_emulated(b, ctx, world, rank, stream.cuda_stream)
            torch.cuda.synchronize(dev)
            for f in OUTS:
                assert torch.equal(a.out[f], b.out[f]), (world, rank, f, ks)
        if ks == [2, 4]:
            assert (a.out["best_k"] == 0).all() and torch.isinf(a.out["obj_value"]).all()
            assert (a.out["obj_value"] > 0).all() and (a.out["status"] == lh.STATUS_INFEASIBLE).all()
        else:
            bk = a.out["best_k"].cpu().numpy()
            ov = a.out["obj_value"].cpu().numpy()
            for f, case in enumerate(cases):
                assert bk[f] > 0 and tc.close(float(ov[f]), tc.objective(case, int(bk[f]))), (case, int(bk[f]))


# ------------------------------------------------------------------ bounded / boxed routes and the many-box launch
BOX_KINDS = ("move2", "cap", "n_off")


def tied_box(case, k, kind):
    """(w_min, w_max, n_min, n_max) of one box: the +-2 box around the rolled optimum, the uniform cap of
    tests/test_gpu_pressure.py's bounded test, or n_max = 0 on every other device."""
    M, W = tc.M_of(case), tc.L_of(case) // k
    if kind == "move2":
        w0 = tc.rolled_w0(case, k)
        return [max(1, v - 2) for v in w0], [min(W, v + 2) for v in w0], None, None
    if kind == "cap":
        return [1] * M, [min(W, -(-W // M) + 1)] * M, None, None
    assert kind == "n_off", kind
    return None, None, None, [0 if i % 2 == 0 else W for i in range(M)]


def boxed_problem(case, k, box):
    p = dict(tc.problem(case, k))
    M = p["M"]
    p["lb"], p["ub"] = p["lb"].copy(), p["ub"].copy()
    lo, hi, nlo, nhi = box
    if lo is not None:
        p["lb"][:M] = np.maximum(p["lb"][:M], lo)
    if hi is not None:
        p["ub"][:M] = np.minimum(p["ub"][:M], hi)
    if nlo is not None:
        p["lb"][M:2 * M] = np.maximum(p["lb"][M:2 * M], nlo)
    if nhi is not None:
        p["ub"][M:2 * M] = np.minimum(p["ub"][M:2 * M], nhi)
    return p


_BOXED = {}


def boxed_answer(case, k, kind):
    """(boxed problem, obj_value or None) of the exact oracle within the box."""
    key = (case, k, kind)
    if key not in _BOXED:
        p = boxed_problem(case, k, tied_box(case, k, kind))
        if (p["lb"] > p["ub"]).any():
            _BOXED[key] = (p, None)
        else:
            st, x, _, _, _ = tc.mo.exact_solve(p)
            assert st in (0, 2), (key, st)
            _BOXED[key] = (p, tc.mo.objective_value(p, x) if st == 0 else None)
    return _BOXED[key]


def check_boxed(r, case, k, kind, what):
    """One HALDAResult (or None) against the oracle within the box; True when the box holds a plan."""
    p, want = boxed_answer(case, k, kind)
    tag = (what, case, k, kind)
    if want is None:
        assert r is None, tag + (r,)
        return False
    M = tc.M_of(case)
    assert r is not None and r.k == k, tag
    assert tc.close(r.obj_value, want), tag + (r.obj_value, want)
    assert sum(r.w) == tc.L_of(case) // k, tag
    v = np.asarray(list(r.w) + list(r.n), float)
    assert (v >= p["lb"][:2 * M]).all() and (v <= p["ub"][:2 * M]).all(), tag + (r.w, r.n)
    got = tc.price(p, r.w, r.n)
    assert got is not None and tc.close(got, want), tag + ("plan prices at", got, "optimum", want)
    return True


@pytest.mark.parametrize("cls,k,routes", [("T64", 1, ("auto",)), ("T16p", 1, ("general", "tables")),
                                          ("T16p", 2, ("general", "tables"))])
def test_bounded_and_boxed_solves_on_tied_fleets(ctx, cls, k, routes):
    """halda_solve_bounded_batch within the +-2 box around the rolled optimum, the uniform cap and an n_max = 0 box
    on every other device: an empty box gives None; else the objective within 1e-9 of the exact oracle's within the
    same column bounds, the plan inside the box and its pinned price at that optimum. On T16p
    halda_solve_boxes_batch over the same boxes equals the route="tables" results entry for entry."""
    from distilp_amd.solver import bounds as bd
    from distilp_amd.solver import boxes as bx

    cases = tc.cases(cls)
    model = tc.model_of(cases[0])
    fleets = [tc.devices(c) for c in cases]
    boxes = [[tied_box(c, k, kind) for c in cases] for kind in BOX_KINDS]
    got = {}
    try:
        for route in routes:
            rs = bd.halda_solve_bounded_batch(fleets * len(BOX_KINDS), model, [b for row in boxes for b in row],
                                              k_candidates=[k], kv_bits=tc.KV_BITS, route=route)
            took = bd.last_bounds_route(ctx)
            print(f"bounded {cls} k = {k} route {route}: took {took}")
            assert took == {"auto": "fused"}.get(route, route), (route, took)
            feasible = 0
            for i, r in enumerate(rs):
                feasible += check_boxed(r, cases[i % len(cases)], k, BOX_KINDS[i // len(cases)], route)
            print(f"bounded {cls} k = {k} route {route}: {feasible} of {len(rs)} boxes hold a plan")
            assert feasible >= len(rs) // 2, (feasible, len(rs))
            got[route] = rs
    finally:
        bd.set_bounds_path(ctx, 0)
    if "tables" in got:
        many = bx.halda_solve_boxes_batch(fleets, model, boxes, k_candidates=[k], kv_bits=tc.KV_BITS)
        print(f"boxes {cls} k = {k}: route {bx.last_boxes_route(ctx)}")
        assert bx.last_boxes_route(ctx) == "tables", bx.last_boxes_route(ctx)
        assert [r for row in many for r in row] == got["tables"]
        for a, b in zip([r for row in many for r in row], got["tables"]):
            assert (a is None) == (b is None) and (a is None or a.obj_value == b.obj_value)


# ------------------------------------------------------------------ budget and change frontiers
P_MOVE = 4


def _pinned_w(case, k):
    from . import budget_cases as bu

    return bu.Pinned(tc.problem(case, k))


@pytest.mark.parametrize("cls,k", tc.FRONTIER_RUNS)
def test_move_frontier_on_tied_fleets(cls, k):
    """halda_move_frontier_batch around the rolled optimum, P = 4: per point the pinned price of the returned plan is
    the reported objective, sum max(0, delta) <= p, moved = sum |delta|, the curve non-increasing and never below the
    free optimum; point 0 is the exact optimum with w pinned to w0 (n free); every point with p >= p* is the free
    optimum. With D = 0 the change kernel's outputs equal the budget kernel's bit for bit."""
    from distilp_amd.solver import budget as bg

    from .test_gpu_change import budget_identity

    cases = tc.cases(cls)
    model = tc.model_of(cases[0])
    fleets = [tc.devices(c) for c in cases]
    w0s = [tc.rolled_w0(c, k) for c in cases]
    incs = [(k, w0, [0] * len(w0)) for w0 in w0s]
    got = bg.halda_move_frontier_batch(fleets, model, incs, 2 * P_MOVE, tc.KV_BITS)
    reached = 0
    for case, w0, pts in zip(cases, w0s, got):
        assert len(pts) == P_MOVE + 1
        free, last = tc.objective(case, k), np.inf
        for p, pt in enumerate(pts):
            tag = (case, k, p)
            assert pt.budget_layers == 2 * p, tag
            if pt.plan is None:
                assert last == np.inf and pt.obj_value == np.inf, tag  # once a plan, always a plan
                assert p < tc.p_star(case, k), tag  # the free optimum is within reach from p* on
                continue
            d = [a - b for a, b in zip(pt.plan.w, w0)]
            assert sum(d) == 0 and sum(v for v in d if v > 0) <= p and pt.moved_layers == sum(abs(v) for v in d), tag
            price = tc.pinned_price(case, k, pt.plan.w, pt.plan.n)
            assert price is not None and tc.close(price, pt.obj_value), tag + (price, pt.obj_value)
            assert pt.obj_value <= last, tag
            assert pt.obj_value >= free - tc.REL_OBJ * max(1.0, abs(free)), tag + (pt.obj_value, free)
            last = pt.obj_value
            if p >= tc.p_star(case, k):
                assert tc.close(pt.obj_value, free), tag + (pt.obj_value, free, tc.p_star(case, k))
                reached += p == P_MOVE
        pin = _pinned_w(case, k)(w0)
        assert (pin is None) == (pts[0].plan is None), (case, k, pin)
        if pin is not None:
            assert tc.close(pts[0].obj_value, pin), (case, k, pts[0].obj_value, pin)
            assert pts[0].plan.w == w0 and pts[0].moved_layers == 0, (case, k)
    print(f"move frontier {cls} k = {k}: {reached} of {len(cases)} fleets reach the free optimum within P = {P_MOVE}")
    assert reached == sum(tc.p_star(c, k) <= P_MOVE for c in cases) >= 1
    budget_identity(model, fleets, k, w0s, P_MOVE, tag=(cls, k))


@pytest.mark.parametrize("k", [1, 2])
def test_failover_frontiers_on_tied_fleets(k):
    """halda_failover_frontiers with device 0 and device M - 1 lost on the T16p fleets, P = 4, the survivors holding
    the rolled optimum: released <= p, loaded = D + released, the pinned price of each plan on the survivors' list
    is the reported objective, the curve non-increasing and never below the list's free optimum."""
    from distilp_amd.solver import change as ch

    model = tc.model(80)
    W = 80 // k
    for case in tc.cases("T16p"):
        devs, w0 = tc.devices(case), tc.rolled_w0(case, k)
        M = len(devs)
        got = ch.halda_failover_frontiers(devs, model, (k, w0, [0] * M), P_MOVE, lost=[0, M - 1], kv_bits=tc.KV_BITS)
        assert len(got) == 2
        for lost, pts in zip((0, M - 1), got):
            keep = [j for j in range(M) if j != lost]
            prob = tc.mo.lower_dense([devs[j] for j in keep], model, k, tc.KV)
            st, xf, _, _, _ = tc.mo.exact_solve(prob)
            free = tc.mo.objective_value(prob, xf) if st == 0 else np.inf
            D, last = W - sum(w0[j] for j in keep), np.inf
            assert D == w0[lost] and len(pts) == P_MOVE + 1
            for p, pt in enumerate(pts):
                tag = (case, k, lost, p)
                assert pt.released_budget == p, tag
                if pt.plan is None:
                    assert last == np.inf and pt.obj_value == np.inf, tag
                    continue
                d = [a - w0[j] for a, j in zip(pt.plan.w, keep)]
                assert sum(pt.plan.w) == W and pt.released == sum(-v for v in d if v < 0) <= p, tag
                assert pt.loaded == sum(v for v in d if v > 0) == D + pt.released, tag
                price = tc.price(prob, pt.plan.w, pt.plan.n)
                assert price is not None and tc.close(price, pt.obj_value), tag + (price, pt.obj_value)
                assert pt.obj_value <= last, tag
                assert pt.obj_value >= free - tc.REL_OBJ * max(1.0, abs(free)), tag + (pt.obj_value, free)
                last = pt.obj_value


# ------------------------------------------------------------------ exact selection
def _same_result(a, b):
    return ((a.k, a.w, a.n, a.sets) == (b.k, b.w, b.n, b.sets)
            and np.float64(a.obj_value).tobytes() == np.float64(b.obj_value).tobytes())


@pytest.mark.parametrize("cls,D", [("T16p", 2), ("T64", 1)])
def test_subset_frontier_on_copies_drops_the_first_indices(ctx, cls, D):
    """On a copies fleet every candidate of one d is the same list of devices, so the values tie bit for bit and the
    strict "<" must keep the earliest: point d drops exactly the first d droppable indices, with keep=None and with
    keep=[0], on subsets path 0 and on the expansion path; its result equals halda_solve_subfleets of that kept list
    bit for bit, and halda_select_devices_exact returns the fewest drops among equal objectives. Path 0 takes the
    fused selection launch (halda_subsets_pick_kernel over one wave per candidate) for the 64-device fleet only: at
    16 devices the host gate expands on both paths, so there the two runs are one route taken twice and only the
    T64 case holds the fused route to the rule."""
    from distilp_amd.solver import halda_select_devices_exact, halda_solve_subfleets, halda_subset_frontier
    from distilp_amd.solver import subsets as ss

    model = tc.model(80)
    ks = list(tc.class_ks(cls))
    for case in tc.cases(cls, kinds=("copies",), scales=(tc.S64,)):
        devs = tc.devices(case)
        M = len(devs)
        for keep in (None, [0]):
            slots = ss.droppable(M, keep)
            by_path = {}
            try:
                for path in (0, 1):
                    ss.set_subsets_path(ctx, path)
                    pts = halda_subset_frontier(devs, model, D, keep, k_candidates=ks, kv_bits=tc.KV_BITS)
                    route = ss.last_subsets_route(ctx)
                    print(f"subsets {cls} keep {keep} path {path}: route {route}")
                    # the default route of a 64-device fleet is the fused selection launch; smaller fleets expand
                    assert route == ("fused" if path == 0 and cls == "T64" else "expand"), (path, route)
                    assert len(pts) == D + 1
                    for d, pt in enumerate(pts):
                        tag = (case, keep, path, d)
                        assert pt.result is not None and pt.dropped == slots[:d], tag + (pt.dropped,)
                        assert pt.kept == [i for i in range(M) if i not in slots[:d]], tag
                        same = halda_solve_subfleets([devs], model, [(0, pt.kept)], ks, kv_bits=tc.KV_BITS)[0]
                        assert _same_result(pt.result, same), tag
                    by_path[path] = pts
                    kept, r = halda_select_devices_exact(devs, model, D, keep, k_candidates=ks, kv_bits=tc.KV_BITS)
                    objs = [pt.obj_value for pt in pts]
                    first = objs.index(min(objs))
                    assert kept == pts[first].kept and _same_result(r, pts[first].result), (case, keep, path)
            finally:
                ss.set_subsets_path(ctx, 0)
            assert by_path[0] == by_path[1], (case, keep)
        full = by_path[0][0].result
        tc.check_plan(case, full.k, full.w, full.n, full.obj_value, "subsets d = 0")


def test_subset_frontier_on_half_fleets_is_the_raw_arg_min():
    """tests/test_gpu_subsets.py's check_frontier (the strict earliest arg-min over every candidate, bit for bit) on
    the T16p half fleets, where each candidate ties with the one that drops the device's twin: both routes."""
    from .test_gpu_subsets import check_frontier

    cases = tc.cases("T16p", kinds=("half",))
    st, obj, dm, bk = check_frontier([tc.devices(c) for c in cases], tc.model(80), 2, ks=list(tc.class_ks("T16p")))
    assert (st[:, 0] == lh.STATUS_OPTIMAL).all() and (dm[:, 0] == 0).all()


# ------------------------------------------------------------------ scale-in and scale-out
def test_scale_in_on_copies_drops_the_first_indices(ctx):
    """halda_scale_in_frontier on a T16p copies fleet, k = 1, w0 = [5] * 16, max_drop 2, max_released 3, at the
    default chunk and with a chunk that holds four candidates (every d >= 1 in several launches): every cell with a
    plan drops exactly the first d devices; each cell's point equals the failover frontier of that list."""
    from distilp_amd.solver import change as ch
    from distilp_amd.solver import scale as sc

    model = tc.model(80)
    case = tc.cases("T16p", kinds=("copies",), scales=(tc.S16,), seeds=(21000,))[0]
    devs = tc.devices(case)
    inc, D, P = (1, [5] * 16, [0] * 16), 2, 3
    runs = []
    try:
        for cap in (0, sc.launch_bytes(16, P, 4)):
            sc.set_change_subsets_chunk(ctx, cap)
            runs.append(sc.halda_scale_in_frontier(devs, model, inc, D, P, kv_bits=tc.KV_BITS))
    finally:
        sc.set_change_subsets_chunk(ctx, 0)
    assert runs[0] == runs[1]
    rows = runs[0]
    assert len(rows) == D + 1 and all(len(r) == P + 1 for r in rows)
    plans = 0
    for d, row in enumerate(rows):
        want = (ch.halda_failover_frontiers(devs, model, inc, P, lost=[tuple(range(d))], kv_bits=tc.KV_BITS)[0] if d
                else ch.halda_change_frontier(devs, model, 1, inc[1], P, kv_bits=tc.KV_BITS))
        for p, cell in enumerate(row):
            if cell.point.plan is None:
                assert want[p].plan is None, (d, p)
                continue
            plans += 1
            assert cell.dropped == list(range(d)) and cell.kept == list(range(d, 16)), (d, p, cell.dropped)
            assert cell.point == want[p], (d, p)
            assert np.float64(cell.point.obj_value).tobytes() == np.float64(want[p].obj_value).tobytes(), (d, p)
    assert plans >= P + 1  # row 0 at the least: the full fleet keeps its plan


def test_scale_out_on_copies_adds_the_last_pool_devices():
    """halda_scale_out_frontier with a pool of three more copies: row a adds the last a pool devices (the candidate
    order is that of the left-out pool indices), and each cell's point equals the change frontier of its list."""
    from distilp_amd.solver import change as ch
    from distilp_amd.solver import scale as sc

    model = tc.model(80)
    case = tc.cases("T16p", kinds=("copies",), scales=(tc.S16,), seeds=(21000,))[0]
    devs = tc.devices(case)
    pool = devs[:3]
    w0, P, q = [5] * 16, 3, 3
    rows = sc.halda_scale_out_frontier(devs, pool, model, (1, w0, [0] * 16), q, P, kv_bits=tc.KV_BITS)
    assert len(rows) == q + 1
    plans = 0
    for a, row in enumerate(rows):
        kept = list(range(16)) + list(range(16 + q - a, 16 + q))
        want = ch.halda_change_frontiers([devs + pool], model, [(0, kept)], 1, [w0 + [0] * a], P, tc.KV_BITS)[0]
        for p, cell in enumerate(row):
            if cell.point.plan is None:
                assert want[p].plan is None, (a, p)
                continue
            plans += 1
            assert cell.added == list(range(q - a, q)) and cell.kept == kept, (a, p, cell.added)
            assert cell.point == want[p], (a, p)
            assert np.float64(cell.point.obj_value).tobytes() == np.float64(want[p].obj_value).tobytes(), (a, p)
    assert plans >= (P + 1) + 1
