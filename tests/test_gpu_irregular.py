"""Irregular device profiles and head placements (tests/irregular_cases.py) on every GPU route, each against
the exact oracle: status, c.x within 1e-9 relative, where the oracle's optimum is unique the w, n, s1, s2, s3 and
t columns of x, the sweep's best k and obj_value, and sets. Every other GPU test has device 0 as the only head
and five clean device kinds; here the head sits on other lanes, in the second 64-device chunk, on several
devices or on none, and the flag bits take the combinations the kinds never give: two VRAM rows on a device, a
GPU row with b forced to 0, beta > 0, coefficients that `put` drops ("Irregular profiles").

A batch has one model and one kv width, so a list of cases is solved group by group (groups()). halda_last_lowered
exposes the GPU-lowered CSR (row_ptr, col_idx, val, row bounds, c, column bounds, integrality), compared bit for
bit with lower_fleet; it does not expose the lowering kernel's `offs`, which are therefore checked through
obj_by_k of the CSR route only."""

import contextlib
import io

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import halda_solve, halda_solve_batch
from distilp_amd.solver import plans as pl
from distilp_amd.solver.batch import assemble, settled_instances
from distilp_amd.solver.fleets import fleet_table, halda_solve_fleets, solve_table
from distilp_amd.solver.lower import lower_fleet
from distilp_amd.solver.subfleets import halda_leave_one_out_batch
from oracle import milp_oracle as mo

from . import irregular_cases as ic
from .conftest import load_json

pytestmark = pytest.mark.gpu

CSR_KERNELS = {"halda_lower_kernel", "halda_screen_kernel", "halda_solve_k1_kernel", "halda_solve_kernel"}


@pytest.fixture(scope="module")
def ctx():
    c = lh.get_context(0)
    yield c
    c.set_fleets_path("fused")
    c.set_timing(False)
    pl.set_plans_path(c, 0)


def groups(case_list):
    """[(model, kv_bits, [cases])]: the cases grouped by the model and kv width they run on, in list order."""
    out = {}
    for c in case_list:
        out.setdefault((id(ic.model_of(c)), c[3]), (ic.model_of(c), c[3], []))[2].append(c)
    return list(out.values())


def repeat_to(cases, n):
    return (cases * (-(-n // len(cases))))[:max(n, len(cases))]


def mixed():
    """Every case of at most 33 devices, the sizes taken in turn."""
    by_m = [ic.cases(Ms=(M,)) for M in (16, 33, 2, 3, 5)]
    out = []
    for i in range(max(len(g) for g in by_m)):
        out += [g[i] for g in by_m if i < len(g)]
    return out


# name: (cases, a kernel that must have run, kernels that must not, repeat each group to this many fleets)
ROUTES = {
    # (a one-fleet register call is served by the resident wave without a launch, so nothing is timed: a group
    # of one fleet is taken twice; halda_solve below goes through that resident wave)
    "register": (lambda: ic.cases(Ms=(64,)), "halda_sweep_kernel", {"halda_sweep_kslot_kernel"}, 2),
    "kslot": (lambda: ic.cases(Ms=(16,)), "halda_sweep_kslot_kernel", {"halda_sweep_kernel"}, 72),
    "m16_tables": (lambda: ic.cases(Ms=(16,)), "halda_sweep_tables_kernel", set(), 0),
    "m33": (lambda: ic.cases(Ms=(33,)), "halda_sweep_tables_kernel", set(), 0),
    "tables": (lambda: ic.cases(Ms=(2, 3, 5)), "halda_sweep_tables_kernel", set(), 0),
    "mixed": (mixed, "halda_sweep_tables_kernel", set(), 0),
    # M = 70 at L = 160: wider than a wave, yet its table slice (about 88 KiB) fits the LDS budget, so this is
    # the table kernel alone on LDS tables; its csr path is what reaches the second chunk of fleet_offsets
    "wide": (lambda: ic.cases(Ms=(70,)), "halda_sweep_tables_kernel", set(), 0),
    # M = 100 at L = 256: tables beyond the LDS budget (BIG_SHAPE, asserted below), so the fused sweep runs
    # halda_sweep_big_kernel and the CSR pipeline halda_solve_big_kernel on global-memory tables.
    # last_fleet_ms reports the big sweep kernel in the table kernel's slot and under its name
    # (include/halda.h), so the name cannot tell the two apart: the shape is what is asserted
    "big": (lambda: ic.cases(Ms=(100,)), "halda_sweep_tables_kernel", set(), 0),
}
# halda_lds_bytes(n_cols, R + 1, table, table_kc) of M = 100, L = 256, k = 1 (tests/test_gpu_shapes.py)
BIG_SHAPE = (7 * 100 + 1, 256 - 100 + 1, 100 * 157, 100 * 29)
LDS_BUDGET = 160 * 1024


def assert_route_shape(ctx, name):
    """The "big" cases' tables exceed the LDS budget and the "wide" cases' do not."""
    if name == "big":
        assert ctx.lib.halda_lds_bytes(*BIG_SHAPE) > LDS_BUDGET
    if name == "wide":
        assert ctx.lib.halda_lds_bytes(7 * 70 + 1, 160 - 70 + 1, 70 * 92, 70 * 12) <= LDS_BUDGET


def sweep(ctx, model, kv, cases, path="fused"):
    """solve_table of the cases' fleets over the model's k list (dense x), and the kernels that ran."""
    table = fleet_table([ic.devices(c) for c in cases], model)
    ctx.set_fleets_path(path)
    ctx.set_timing(True)
    try:
        res = solve_table(table, model, list(ic.ks_all(cases[0][0])), ic.kv_factor(kv), want_x=True)
        ran = set(ctx.last_fleet_ms())
    finally:
        ctx.set_fleets_path("fused")
        ctx.set_timing(False)
    return table, res, ran


def check_sweep(cases, table, res, what):
    """A FleetSolve (dense x) against the oracle: per (fleet, k) the status, x and obj_by_k; per fleet the best
    k by the reference's strict "<", obj_value and (w, n)."""
    for f, case in enumerate(cases):
        M, L = case[0], ic.L_of(case[0])
        a = int(table.dev_off[f])
        best = None
        for j, k in enumerate(res.ks):
            if L // k < M:
                assert res.status[f, j] == lh.STATUS_INFEASIBLE and np.isinf(res.obj_by_k[f, j]), (what, case, k)
                continue
            st = ic.exact(case, k)[0]
            if st != 0:
                assert st == 2 and res.status[f, j] == lh.STATUS_INFEASIBLE, (what, case, k, st)
                continue
            assert res.status[f, j] == lh.STATUS_OPTIMAL, (what, case, k, res.status[f, j])
            x = res.x[f, j, :7 * M + 1]
            ic.check_x(x, case, k, what)
            obj = mo.objective_value(ic.problem(case, k), x)
            assert ic.close(float(res.obj_by_k[f, j]), obj) and ic.close(obj, ic.objective(case, k)), (
                what, case, k, float(res.obj_by_k[f, j]), obj, ic.objective(case, k))
            if best is None or obj < best[0]:
                best = (obj, k, x)
        assert best is not None and res.best_k[f] == best[1], (what, case, int(res.best_k[f]), best[1])
        assert ic.close(float(res.obj_value[f]), best[0]), (what, case)
        assert np.array_equal(res.w[a:a + M], best[2][:M]) and np.array_equal(res.n[a:a + M], best[2][M:2 * M]), (
            what, case)
        if ic.best_k_is_clear(case):
            assert res.best_k[f] == ic.best_k(case)[0], (what, case, int(res.best_k[f]), ic.best_k(case))
        assert table.sets(f) == mo.sets_of(ic.devices(case)), (what, case)


def as_oracle(r, case, what=""):
    """A HALDAResult of a case's fleet against the oracle's k-sweep: k, obj_value, sets and, where unique, w, n."""
    M = case[0]
    kb, ob = ic.best_k(case)
    assert r is not None and ic.close(r.obj_value, ob), (what, case, r, kb, ob)
    assert r.sets == mo.sets_of(ic.devices(case)), (what, case)
    if ic.best_k_is_clear(case):
        assert r.k == kb, (what, case, r.k, kb)
        if ic.unique(case, kb):
            xo = ic.exact(case, kb)[1]
            assert r.w == [int(v) for v in xo[:M]] and r.n == [int(v) for v in xo[M:2 * M]], (what, case, r)


# ------------------------------------------------------------------ the fused sweep, each shape's own route
@pytest.mark.parametrize("name", list(ROUTES))
def test_fused_sweep_equals_the_oracle(ctx, name):
    make, must, must_not, rep = ROUTES[name]
    assert_route_shape(ctx, name)
    for model, kv, cases in groups(make()):
        batch = repeat_to(cases, rep) if rep else cases
        table, res, ran = sweep(ctx, model, kv, batch)
        print(f"{name} / {kv}: {len(batch)} fleets ({len(cases)} distinct), kernels {sorted(ran)}")
        assert ran and not (ran & CSR_KERNELS), ran
        assert must in ran and not (ran & must_not), (name, ran)
        check_sweep(batch, table, res, f"{name} / {kv}")
        if name == "mixed":
            continue
        # the Python entries: the batch call and one halda_solve per fleet give the same answers
        fleets = [ic.devices(c) for c in cases]
        many = halda_solve_fleets(fleets, model, mip_gap=1e-4, kv_bits=kv)
        for case, devs, r in zip(cases, fleets, many):
            as_oracle(r, case, f"{name} halda_solve_fleets")
            with contextlib.redirect_stdout(io.StringIO()):
                one = halda_solve(devs, model, mip_gap=1e-4, plot=False, kv_bits=kv)
            assert one.sets == r.sets, (name, case)
            if ic.best_k_is_clear(case) and ic.unique(case, ic.best_k(case)[0]):
                assert (one.k, one.w, one.n) == (r.k, r.w, r.n), (name, case, one, r)
            assert ic.close(one.obj_value, r.obj_value), (name, case, one.obj_value, r.obj_value)


# ------------------------------------------------------------------ forced DP, lowering kernel + CSR pipeline
def check_lowered_csr(cases, model, kv, ks):
    """The batch the lowering kernel left on the device (halda_last_lowered) against lower_fleet, bit for bit:
    row_ptr, col_idx, val, c, column bounds, integrality and row bounds of every (fleet, k)."""
    from .test_gpu_fleets import _d2h, _lowered

    b = _lowered()
    n = b.n_inst
    assert n == len(cases) * len(ks)
    n_cols, n_rows = _d2h(b.n_cols, n, np.int32), _d2h(b.n_rows, n, np.int32)
    csr_off, col_off, row_off = (_d2h(getattr(b, f), n, np.int64) for f in ("csr_off", "col_off", "row_off"))
    seen = set()
    for fi, case in enumerate(cases):
        if case in seen:
            continue
        seen.add(case)
        M = case[0]
        fl = lower_fleet(ic.devices(case), model, kv)
        for j, k in enumerate(ks):
            i = fi * len(ks) + j
            m = int(n_rows[i])
            assert (n_cols[i], m) == (fl.n_cols, fl.n_rows), (case, k, n_cols[i], m, fl.n_cols, fl.n_rows)
            rp = _d2h(b.row_ptr + 4 * int(csr_off[i]), m + 1, np.int32)
            assert np.array_equal(np.diff(rp), np.diff(fl.row_ptr)), (case, k, "row_ptr")
            cols = _d2h(b.col_idx + 4 * int(rp[0]), int(rp[-1] - rp[0]), np.int32)
            vals = _d2h(b.val + 8 * int(rp[0]), int(rp[-1] - rp[0]), np.float64)
            assert np.array_equal(cols, fl.col_idx) and np.array_equal(vals, fl.val), (case, k, "col_idx / val")
            c, lb, ub, rlb, rub, integ, W = fl.instance(k)
            co, ro = int(col_off[i]), int(row_off[i])
            if W < M:  # bound-infeasible: only what the screen reads is lowered
                assert np.array_equal(_d2h(b.col_lb + 8 * co, M, np.float64), lb[:M])
                assert np.array_equal(_d2h(b.col_ub + 8 * co, M, np.float64), ub[:M])
                continue
            assert np.array_equal(_d2h(b.c + 8 * co, fl.n_cols, np.float64), c), (case, k, "c")
            assert np.array_equal(_d2h(b.col_lb + 8 * co, fl.n_cols, np.float64), lb), (case, k, "lb")
            assert np.array_equal(_d2h(b.col_ub + 8 * co, fl.n_cols, np.float64), ub), (case, k, "ub")
            assert np.array_equal(_d2h(b.integrality + co, fl.n_cols, np.uint8), integ), (case, k)
            assert np.array_equal(_d2h(b.row_lb + 8 * ro, m, np.float64), rlb), (case, k, "row_lb")
            assert np.array_equal(_d2h(b.row_ub + 8 * ro, m, np.float64), rub), (case, k, "row_ub")


@pytest.mark.parametrize("name", ["register", "kslot", "m33", "tables", "mixed", "wide", "big"])
def test_forced_dp_and_csr_paths_equal_the_oracle_and_each_other(ctx, name):
    """The same tables with the exact DP forced for every k = 1 solve ("dp") and through the lowering kernel
    and the CSR pipeline ("csr"): each against the oracle; status, best k, w and n equal among the three; the
    lowered CSR equal to the host lowering bit for bit (the two-row VRAM path and the zero-dropping put)."""
    make, _, _, rep = ROUTES[name]
    assert_route_shape(ctx, name)
    for model, kv, cases in groups(make()):
        batch = repeat_to(cases, rep) if rep else cases
        runs = {}
        for path in ("fused", "dp", "csr"):
            table, res, ran = sweep(ctx, model, kv, batch, path)
            print(f"{name} / {kv} / {path}: kernels {sorted(ran)}")
            if path == "csr":
                assert "halda_lower_kernel" in ran, ran
                check_lowered_csr(batch, model, kv, res.ks)
            check_sweep(batch, table, res, f"{name} / {kv} / {path}")
            runs[path] = res
        for path in ("dp", "csr"):
            for f in ("status", "best_k", "w", "n"):
                assert np.array_equal(getattr(runs[path], f), getattr(runs["fused"], f)), (name, kv, path, f)


# ------------------------------------------------------------------ the CSR pipeline on host-lowered batches
@pytest.mark.parametrize("Ms", [(64,), (16,), (33, 2, 3, 5), (70,), (100,)])
def test_csr_pipeline_on_host_lowered_batches(ctx, Ms):
    """get_context(0).solve(assemble([lower_fleet(...)])) -- the screen kernel, the persistent k = 1 kernel and
    the general kernel -- and the same batch with the settled flags, each against the oracle. One batch holds
    every model and kv width of the list (a lowered fleet carries its own)."""
    import torch

    from .test_gpu_settled import _device_solve

    cases = ic.cases(Ms=Ms)
    lowered = [lower_fleet(ic.devices(c), ic.model_of(c), c[3]) for c in cases]
    b, refs = assemble(lowered, [list(ic.ks_all(c[0])) for c in cases])
    res = ctx.solve(b)
    dev = torch.device("cuda", 0)
    settled = _device_solve(ctx, b, settled_instances(b), dev, torch.cuda.Stream(dev))
    solved = 0
    for idx, ref in enumerate(refs):
        case, k = cases[ref.fleet], ref.k
        st = ic.exact(case, k)[0] if ic.L_of(case[0]) // k >= case[0] else 2
        for what, status, xs, obj_lin in (("solve", res.status, res.x, res.obj_lin),
                                          ("settled", settled["status"], settled["x"], settled["obj_lin"])):
            if st != 0:
                assert status[idx] == lh.STATUS_INFEASIBLE, (what, case, k)
                continue
            assert status[idx] == lh.STATUS_OPTIMAL, (what, case, k, int(status[idx]))
            assert ic.close(float(obj_lin[idx]), ic.exact(case, k)[2]), (what, case, k)
            ic.check_x(xs[ref.col_off:ref.col_off + ref.n_cols], case, k, what)
        solved += st == 0
    assert solved == len(ic.instances(cases))


# ------------------------------------------------------------------ resident tables
def check_resident(cases, table, dt, ks, what):
    """A resident table's outputs (no x) against the oracle: status, obj_by_k, best k, obj_value, (w, n)."""
    out = {k: v.cpu().numpy() for k, v in dt.out.items()}
    nk = len(ks)
    for f, case in enumerate(cases):
        M, a = case[0], int(table.dev_off[f])
        for j, k in enumerate(ks):
            st = ic.exact(case, k)[0] if ic.L_of(M) // k >= M else 2
            if st != 0:
                assert out["status"][f * nk + j] == lh.STATUS_INFEASIBLE, (what, case, k)
                continue
            assert out["status"][f * nk + j] == lh.STATUS_OPTIMAL, (what, case, k)
            assert ic.close(float(out["obj_by_k"][f * nk + j]), ic.objective(case, k)), (what, case, k)
        kb, ob = ic.best_k(case)
        assert ic.close(float(out["obj_value"][f]), ob), (what, case)
        if ic.best_k_is_clear(case):
            assert out["best_k"][f] == kb, (what, case, int(out["best_k"][f]), kb)
            if ic.unique(case, kb):
                xo = ic.exact(case, kb)[1]
                assert np.array_equal(out["w"][a:a + M], xo[:M]) and np.array_equal(out["n"][a:a + M], xo[M:2 * M]), (
                    what, case)


def test_resident_tables_and_group_launches(ctx):
    """DeviceFleetTable.launch on the mixed table; the steps kernel over two resident M = 64 tables; the
    k-slot group launch over two 72-fleet M = 16 tables: every table's outputs against the oracle.
    last_fleet_ms has no name for halda_sweep_steps_kernel: a persistent group of register-only tables is
    the launch that runs it, reported in the register kernel's slot, so group.persistent and that slot alone
    are what is asserted for M = 64."""
    import torch

    from distilp_amd.solver.fleets import DeviceFleetTable, PlanGroup

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)

    def resident(cases, model, kv):
        table = fleet_table([ic.devices(c) for c in cases], model)
        ks = list(ic.ks_all(cases[0][0]))
        return table, DeviceFleetTable(table, model, ks, ic.kv_factor(kv), dev, want_per_k=True), ks

    model, kv, cases = groups(mixed())[0]
    table, dt, ks = resident(cases, model, kv)
    dt.launch(ctx, stream.cuda_stream)
    torch.cuda.synchronize(dev)
    check_resident(cases, table, dt, ks, "launch / mixed")

    for M, n, kernel in ((64, 0, "halda_sweep_kernel"), (16, 72, "halda_sweep_kslot_kernel")):
        model, kv, cases = groups(ic.cases(Ms=(M,), kvs=("4bit",)))[0]
        assert len(cases) >= 5
        sets = [repeat_to(cases, n) if n else cases, repeat_to(cases[::-1], n) if n else cases[::-1]]
        tabs = [resident(cs, model, kv) for cs in sets]
        group = PlanGroup([dt for _, dt, _ in tabs], ctx)
        assert group.persistent
        for _, dt, _ in tabs:
            for v in dt.out.values():
                v.zero_()
        torch.cuda.synchronize(dev)
        ctx.set_timing(True)
        try:
            group.launch(1, 5, stream.cuda_stream)
            torch.cuda.synchronize(dev)
            ran = set(ctx.last_fleet_ms())
        finally:
            ctx.set_timing(False)
        print(f"group launch M = {M}: kernels {sorted(ran)}")
        assert kernel in ran and (M != 64 or ran == {kernel}), ran
        for cs, (table, dt, ks) in zip(sets, tabs):
            check_resident(cs, table, dt, ks, f"group M = {M}")
        group.close()


# ------------------------------------------------------------------ sub-fleets
@pytest.mark.parametrize("edit,M", [("two_heads", 16), ("head_at:last", 16), ("no_head", 16), ("two_heads", 64)])
def test_leave_one_out_with_moved_heads(edit, M):
    """halda_leave_one_out_batch on a fleet with two heads (dropping device 0 leaves the later head), with the
    head last (dropping it leaves none) and with no head, against halda_solve_batch of the materialised lists
    (pydantic ==) and, for the lists that drop device 0, the head and the last device, the exact oracle."""
    case = next(c for c in ic.cases(Ms=(M,)) if edit in c[4])
    devs, model, kv = ic.devices(case), ic.model_of(case), case[3]
    got = halda_leave_one_out_batch([devs], model, kv_bits=kv)[0]
    lists = [devs[:i] + devs[i + 1:] for i in range(M)]
    assert got == halda_solve_batch(lists, model, kv_bits=kv), (edit, M)
    head = next((i for i, d in enumerate(devs) if d.is_head), 0)
    for i in sorted({0, head, M - 1}):
        want, per_k = mo.halda_solve_oracle(lists[i], model, mip_gap=1e-4, kv_bits=kv, solver="exact")
        r = got[i]
        assert r is not None and ic.close(r.obj_value, want["obj_value"]), (edit, M, i, r, want)
        assert r.sets == want["sets"]
        objs = sorted(q["obj_value"] for q in per_k if q["success"])
        rec = next(q for q in per_k if q["k"] == want["k"])
        tol = 1e-7 * max(1.0, abs(rec["obj_value"]))
        if rec["margin"] > tol and (len(objs) < 2 or objs[1] - objs[0] > tol):
            assert (r.k, r.w, r.n) == (want["k"], want["w"], want["n"]), (edit, M, i, r, want)


# ------------------------------------------------------------------ variants
@pytest.mark.parametrize("M,route", [(64, "fused"), (5, "fused")])
def test_variants_on_irregular_fleets(M, route):
    """halda_solve_variants over kv 4bit / 8bit / fp16 equals one halda_solve_fleets call per variant, bit for
    bit (tests/test_gpu_variants.py's check_variants, which asserts the route); the 4bit variant's first fleet
    against the oracle."""
    from distilp_amd.solver import halda_solve_variants

    from .test_gpu_variants import check_variants

    model, kv, cases = groups(ic.cases(Ms=(M,), kvs=("4bit",)))[0]
    fleets = [ic.devices(c) for c in cases]
    variants = [(model, "4bit"), (model, "8bit"), (model, "fp16")]
    check_variants(fleets, variants, paths=((0, route),))
    got = halda_solve_variants(fleets[:1], variants)
    as_oracle(got[0][0], cases[0], "variants")


# ------------------------------------------------------------------ plans
def plans_of(cases, rng):
    """[(case, k, w, n, feasible, obj_value)]: the oracle's optimum of every instance and its two neighbours,
    priced by evaluate_plan_np (held to the oracle and to HiGHS by tests/test_irregular.py)."""
    out = []
    for c in cases:
        M, model = c[0], ic.model_of(c)
        t = fleet_table([ic.devices(c)], model)
        for k in ic.ks_of(M):
            st, xo, _, _ = ic.exact(c, k)
            if st != 0:
                continue
            w, n = [int(v) for v in np.rint(xo[:M])], [int(v) for v in np.rint(xo[M:2 * M])]
            out.append((c, k, w, n, True, ic.objective(c, k)))
            for _, w2, n2 in ic.neighbours(rng, w, n):
                e = pl.evaluate_plan_np(t, model, 0, k, w2, n2, 0.5)
                out.append((c, k, w2, n2, e.feasible, e.obj_value))
    return out


def test_plans_on_the_gpu_equal_the_numpy_specification():
    """halda_evaluate_plans_batch on the oracle's optima and their neighbours of every kv 4bit case: status,
    objective within 1e-9, reason, bottleneck and cycle_time equal to evaluate_plan_np; the optima feasible at
    the oracle's objective."""
    from .test_gpu_plans import _check_against_np

    rng = np.random.default_rng(ic.pc.NEIGHBOUR_SEED)
    total = 0
    for model, kv, cases in groups(ic.cases(kvs=("4bit",))):
        plans = plans_of(cases, rng)
        _check_against_np([(c, ic.devices(c), k, w, n, ok, obj) for c, k, w, n, ok, obj in plans], model)
        total += len(plans)
    assert total >= 300


@pytest.mark.parametrize("path,M,rep", [(0, 64, 0), (2, 64, 0), (0, 16, 72), (2, 16, 72)])
def test_sweep_with_incumbents_on_both_plan_paths(ctx, path, M, rep):
    """halda_solve_fleets_plans on the default path and on halda_set_plans_path(ctx, 2): the sweep against the
    oracle, the evaluation of each fleet's k = 1 neighbour plan against evaluate_plan_np."""
    model, kv, cases = groups(ic.cases(Ms=(M,), kvs=("4bit",)))[0]
    rng = np.random.default_rng(ic.pc.NEIGHBOUR_SEED)
    first = {}
    for c in cases:
        xo = ic.exact(c, 1)[1]
        w, n = [int(v) for v in np.rint(xo[:M])], [int(v) for v in np.rint(xo[M:2 * M])]
        _, w2, n2 = ic.neighbours(rng, w, n)[0]
        first[c] = (1, w2, n2)
    batch = repeat_to(cases, rep) if rep else cases
    table = fleet_table([ic.devices(c) for c in batch], model)
    ks = list(ic.ks_all(M))
    k, w, n = pl._plan_arrays(table, [first[c] for c in batch], allow_none=False)
    pl.set_plans_path(ctx, path)
    try:
        res, buf = pl.solve_plans_table(table, model, ks, k, w, n, 0.5)
        route = pl.last_plans_route(ctx)
    finally:
        pl.set_plans_path(ctx, 0)
    print(f"M = {M} path {path}: route {route}")
    assert route in ("fused", "two_launch"), route
    nk = len(ks)
    for f, case in enumerate(batch):
        e = pl.evaluate_plan_np(table, model, f, *first[case], 0.5)
        assert (buf.status[f], buf.reason[f], buf.bottleneck[f]) == (e.status, e.reason, e.bottleneck), (case, e)
        if e.feasible:
            assert buf.cycle[f] == e.cycle and ic.close(float(buf.obj[f]), e.obj_value), case
        for j, kk in enumerate(ks):
            off = int(res.x_off[f * nk + j])
            if ic.L_of(M) // kk < M:
                assert off == -1 and res.status[f, j] == lh.STATUS_INFEASIBLE
                continue
            assert res.status[f, j] == lh.STATUS_OPTIMAL, (case, kk)
            ic.check_x(res.x[off:off + 7 * M + 1], case, kk, f"plans path {path}")
        assert ic.close(float(res.obj_value[f]), ic.best_k(case)[1]), case
        if ic.best_k_is_clear(case):
            assert res.best_k[f] == ic.best_k(case)[0], case


# ------------------------------------------------------------------ bounds
@pytest.mark.parametrize("M,k,route,ask", [(64, 1, "fused", "auto"), (16, 1, "general", "general"),
                                           (16, 2, "tables", "tables"), (16, 4, "general", "general")])
def test_bounded_sweep_on_irregular_fleets(ctx, M, k, route, ask):
    """halda_solve_bounded_batch within the D = 2 move box around the oracle's own optimum and within the
    uniform cap: against the exact oracle on the dense problem with the w columns' bounds narrowed."""
    model, kv, cases = groups(ic.cases(Ms=(M,), kvs=("4bit",)))[0]
    W = ic.L_of(M) // k
    fleets, boxes, kinds = [], [], []
    for case in cases:
        w0 = [int(v) for v in np.rint(ic.exact(case, k)[1][:M])]
        for kind, box in ((2, ([max(1, v - 2) for v in w0], [min(W, v + 2) for v in w0])),
                          ("cap", ([1] * M, [min(W, -(-W // M) + 1)] * M))):
            fleets.append(ic.devices(case))
            boxes.append(box)
            kinds.append((case, kind))
    got = bd.halda_solve_bounded_batch(fleets, model, boxes, k_candidates=[k], kv_bits=kv, route=ask)
    assert bd.last_bounds_route(ctx) == route, bd.last_bounds_route(ctx)
    feasible = 0
    for (case, kind), (lo, hi), r in zip(kinds, boxes, got):
        p = dict(ic.problem(case, k))
        p["lb"], p["ub"] = p["lb"].copy(), p["ub"].copy()
        p["lb"][:M], p["ub"][:M] = lo, hi
        st, xo, b1, b2, _ = mo.exact_solve(p)
        if st != 0:
            assert st == 2 and r is None, (case, kind, r)
            continue
        feasible += 1
        assert r is not None and r.k == k, (case, kind)
        assert ic.close(r.obj_value, mo.objective_value(p, xo)), (case, kind, r.obj_value, mo.objective_value(p, xo))
        assert all(a <= v <= b for a, v, b in zip(lo, r.w, hi)), (case, kind)
        if mo.uniqueness_margin_ok(b1, b2):
            assert r.w == [int(v) for v in xo[:M]] and r.n == [int(v) for v in xo[M:2 * M]], (case, kind, r)
    print(f"bounded M = {M} k = {k}: {feasible} of {len(got)} feasible")
    assert feasible >= len(cases)  # the move box around the optimum holds the optimum


# ------------------------------------------------------------------ the reference's recorded results
def test_python_entries_match_the_recorded_irregular_results():
    """halda_solve_batch (one call per model) and halda_solve on the fleets of tests/golden/irregular.json
    against the reference's recorded HALDAResult, under the standing rule (tests/subfleets_cases.py)."""
    from .subfleets_cases import result_mismatch

    recs = {ic.case_of_record(r): r for r in load_json("irregular.json")["fleets"]}
    for model, kv, cases in groups(list(recs)):
        fleets = [ic.devices(c) for c in cases]
        got = halda_solve_batch(fleets, model, mip_gap=1e-4, kv_bits="4bit")
        for case, devs, r in zip(cases, fleets, got):
            rec = recs[case]
            assert rec["error"] is None
            per_k = ic.exact_sweep(case)[1]
            assert result_mismatch(r, rec, per_k) is None, (case, result_mismatch(r, rec, per_k))
            with contextlib.redirect_stdout(io.StringIO()):
                one = halda_solve(devs, model, mip_gap=1e-4, plot=False, kv_bits="4bit")
            assert result_mismatch(one, rec, per_k) is None, (case, result_mismatch(one, rec, per_k))
