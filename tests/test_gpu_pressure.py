"""Memory-pressured fleets (tests/pressure_cases.py) on every GPU route, each against the exact oracle: status,
c.x within 1e-9 relative, and -- where the oracle's optimum is unique -- the w, n, s1, s2, s3 and t columns of x.
On the unscaled synthetic fleets of 16 and 64 devices every slack is 0 and every n sits at a bound, so the
least-slack rule, the kinks of g_i(w, n), the n*(w) search, the convexity re-check and the slack bound decide
nothing there; here they decide nearly every optimum ("Memory pressure")."""

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import halda_solve, halda_solve_batch, halda_solve_variants
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import plans as pl
from distilp_amd.solver.batch import assemble, settled_instances
from distilp_amd.solver.fleets import fleet_table, solve_table
from distilp_amd.solver.lower import lower_fleet
from distilp_amd.solver.subfleets import halda_leave_one_out_batch
from oracle import milp_oracle as mo

from . import pressure_cases as pc
from .conftest import load_json

pytestmark = pytest.mark.gpu

KS = list(pc.KS)
L = pc.L


@pytest.fixture(scope="module")
def ctx():
    c = lh.get_context(0)
    yield c
    c.set_fleets_path("fused")
    c.set_timing(False)
    pl.set_plans_path(c, 0)


def devs_of(case):
    return pc.devices(case[2], case[0], case[1])


def batch(Ms, kv="4bit", seeds=None):
    return pc.cases(Ms=Ms, kvs=(kv,), seeds=seeds)


def kslot_batch(kv="4bit"):
    """The M = 16 cases three times over: the k-slot kernel takes batches of more than 64 fleets (smaller
    ones run the table kernel alone), and the case list has 32 distinct 16-device fleets at kv 4bit (8 at
    fp16, taken nine times)."""
    cs = batch((16,), kv)
    return cs * (3 if kv == "4bit" else 9)


def interleaved(kv="4bit"):
    """One mixed-size batch: the M = 64, 16, 33, 2, 3 and 5 cases taken in turn (32 fleets)."""
    groups = [batch((M,), kv, range(6 if M in (64, 16) else 4)) for M in (64, 16, 33, 2, 3, 5)]
    out = []
    for i in range(max(len(g) for g in groups)):
        out += [g[i] for g in groups if i < len(g)]
    return out[:32]


def sweep(ctx, cases, path="fused", want_x=True):
    """solve_table of the cases' fleets over every k of 80, and the kernels that ran."""
    model = pc.our_model()
    table = fleet_table([devs_of(c) for c in cases], model)
    ctx.set_fleets_path(path)
    ctx.set_timing(True)
    try:
        res = solve_table(table, model, KS, pc.kv_factor(cases[0][3]), want_x=want_x)
        ran = set(ctx.last_fleet_ms())
    finally:
        ctx.set_fleets_path("fused")
        ctx.set_timing(False)
    return table, res, ran


def check_sweep(cases, table, res, what):
    """A FleetSolve over KS (dense x) against the oracle: per (fleet, k) the status, x and obj_by_k; per fleet
    the best k by the reference's strict "<", obj_value and (w, n)."""
    n_unique = 0
    for f, case in enumerate(cases):
        M = case[0]
        a = int(table.dev_off[f])
        best = None
        for j, k in enumerate(KS):
            if L // k < M:
                assert res.status[f, j] == lh.STATUS_INFEASIBLE and np.isinf(res.obj_by_k[f, j]), (what, case, k)
                continue
            st = pc.exact(case, k)[0]
            if st != 0:
                assert st == 2 and res.status[f, j] == lh.STATUS_INFEASIBLE, (what, case, k, st)
                continue
            assert res.status[f, j] == lh.STATUS_OPTIMAL, (what, case, k, res.status[f, j])
            x = res.x[f, j, :7 * M + 1]
            pc.check_x(x, case, k, what)
            n_unique += pc.unique(case, k)
            obj = mo.objective_value(pc.problem(case, k), x)
            assert pc.close(float(res.obj_by_k[f, j]), obj) and pc.close(obj, pc.objective(case, k)), (what, case, k)
            if best is None or obj < best[0]:
                best = (obj, k, x)
        assert best is not None and res.best_k[f] == best[1], (what, case, int(res.best_k[f]), best[1])
        assert pc.close(float(res.obj_value[f]), best[0]), (what, case)
        assert np.array_equal(res.w[a:a + M], best[2][:M]) and np.array_equal(res.n[a:a + M], best[2][M:2 * M]), (
            what, case)
        ok = pc.best_k(case, [k for k in KS if L // k >= M])
        gaps = sorted(pc.objective(case, k) for k in KS if L // k >= M and pc.exact(case, k)[0] == 0)
        if len(gaps) < 2 or gaps[1] - gaps[0] > 1e-7 * max(1.0, abs(gaps[0])):
            assert res.best_k[f] == ok[0], (what, case, int(res.best_k[f]), ok)
    return n_unique


SWEEPS = {
    "register": (lambda: batch((64,)), {"halda_sweep_kernel"}),
    "kslot": (kslot_batch, {"halda_sweep_kslot_kernel"}),
    "m16_tables": (lambda: batch((16,)), {"halda_sweep_tables_kernel"}),
    "m33": (lambda: batch((33,)), None),
    "tables": (lambda: batch((2, 3, 5)), None),
    "mixed": (interleaved, None),
    "register_fp16": (lambda: batch((64,), "fp16"), {"halda_sweep_kernel"}),
    "kslot_fp16": (lambda: kslot_batch("fp16"), {"halda_sweep_kslot_kernel"}),
}


@pytest.mark.parametrize("name", list(SWEEPS))
def test_fused_sweep_equals_the_oracle(ctx, name):
    make, want_kernels = SWEEPS[name]
    cases = make()
    assert 1 <= len(set(cases)) <= 32
    table, res, ran = sweep(ctx, cases)
    print(f"{name}: {len(cases)} fleets, kernels {sorted(ran)}")
    csr = {"halda_lower_kernel", "halda_screen_kernel", "halda_solve_k1_kernel", "halda_solve_kernel"}
    assert ran and not (ran & csr), ran  # a fused route, not the CSR pipeline
    if want_kernels is not None:
        assert want_kernels <= ran, (name, ran)
    if name.startswith("register"):
        assert "halda_sweep_kslot_kernel" not in ran and "halda_sweep_tables_kernel" not in ran, ran
    n_unique = check_sweep(cases, table, res, name)
    assert n_unique >= 0.95 * sum(1 for c in cases for k in KS if L // k >= c[0])
    if name.startswith("kslot"):
        assert "halda_sweep_kernel" not in ran, ran


@pytest.mark.parametrize("name", ["register", "kslot", "m33", "tables", "mixed"])
def test_forced_dp_and_csr_paths_equal_the_oracle_and_each_other(ctx, name):
    """The same tables with the exact DP forced for every k = 1 solve ("dp") and through the lowering kernel
    and the CSR pipeline ("csr"): each against the oracle; status, best k, w and n equal among the three."""
    cases = SWEEPS[name][0]()
    runs = {}
    for path in ("fused", "dp", "csr"):
        table, res, ran = sweep(ctx, cases, path)
        print(f"{name} / {path}: kernels {sorted(ran)}")
        if path == "csr":
            assert "halda_lower_kernel" in ran, ran
        check_sweep(cases, table, res, f"{name} / {path}")
        runs[path] = res
    for path in ("dp", "csr"):
        for f in ("status", "best_k", "w", "n"):
            assert np.array_equal(getattr(runs[path], f), getattr(runs["fused"], f)), (name, path, f)


@pytest.mark.parametrize("name", ["register", "kslot"])
def test_sweeps_are_deterministic(ctx, name):
    cases = SWEEPS[name][0]()
    a = sweep(ctx, cases)[1]
    b = sweep(ctx, cases)[1]
    for f in ("best_k", "obj_value", "w", "n", "obj_by_k", "status", "x", "c"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (name, f)


# ------------------------------------------------------------------ the CSR pipeline on host-lowered batches
@pytest.mark.parametrize("Ms", [(64,), (16,), (33, 2, 3, 5)])
def test_csr_pipeline_on_host_lowered_batches(ctx, Ms):
    """get_context(0).solve(assemble([lower_fleet(...)])) -- the screen kernel, the persistent k = 1 kernel and
    the general kernel -- and the same batch with the settled flags (halda_solve_k1_settled_kernel), each
    against the oracle. res.nodes is the count of DP passes: 1 + the events of the incremental threshold scan
    (or, had a leaf failed the convexity / monotonicity re-check, the passes of the DP-per-candidate scan: the
    count cannot tell the two apart, so the optimum is required either way and the counts are printed)."""
    import torch

    from .test_gpu_settled import _device_solve

    cases = batch(Ms, seeds=range(8))
    model = pc.our_model()
    lowered = [lower_fleet(devs_of(c), model, "4bit") for c in cases]
    b, refs = assemble(lowered, [KS] * len(lowered))
    res = ctx.solve(b)
    dev = torch.device("cuda", 0)
    flags = settled_instances(b)
    settled = _device_solve(ctx, b, flags, dev, torch.cuda.Stream(dev))
    nodes = {}
    for idx, ref in enumerate(refs):
        case, k = cases[ref.fleet], ref.k
        st = pc.exact(case, k)[0] if L // k >= case[0] else 2
        for what, status, xs, obj_lin, nd in (("solve", res.status, res.x, res.obj_lin, res.nodes),
                                              ("settled", settled["status"], settled["x"], settled["obj_lin"],
                                               settled["nodes"])):
            msg = (what, case, k, "nodes", int(nd[idx]))
            if st != 0:
                assert status[idx] == lh.STATUS_INFEASIBLE, msg
                continue
            assert status[idx] == lh.STATUS_OPTIMAL, msg + (int(status[idx]),)
            assert pc.close(float(obj_lin[idx]), pc.exact(case, k)[2]), msg
            try:
                pc.check_x(xs[ref.col_off:ref.col_off + ref.n_cols], case, k, what)
            except AssertionError as e:
                raise AssertionError(f"{msg}: {e}") from None
        if st == 0:
            assert int(res.nodes[idx]) == int(settled["nodes"][idx])
            nodes[(case, k)] = int(res.nodes[idx])
    multi = {q: v for q, v in nodes.items() if q[1] > 1 and v >= 3}  # phase 0 + more than one event
    hist = np.bincount([min(v, 9) for q, v in nodes.items() if q[1] > 1], minlength=10).tolist()
    print(f"M {Ms}: {len(nodes)} solved instances; k > 1 passes histogram (9 = 9 or more) {hist}; "
          f"{len(multi)} scans of more than one event")
    if any(L // 2 >= M for M in Ms):
        assert multi, nodes


# ------------------------------------------------------------------ steps / group launch
def _resident(cases, kv, dev, per_k=True):
    from distilp_amd.solver.fleets import DeviceFleetTable

    model = pc.our_model()
    table = fleet_table([devs_of(c) for c in cases], model)
    return table, DeviceFleetTable(table, model, KS, kv, dev, want_per_k=per_k)


def check_resident(cases, table, dt, what):
    """A resident table's outputs (no x) against the oracle: status, obj_by_k, best k, obj_value, (w, n)."""
    out = {k: v.cpu().numpy() for k, v in dt.out.items()}
    nk = len(KS)
    for f, case in enumerate(cases):
        M, a = case[0], int(table.dev_off[f])
        for j, k in enumerate(KS):
            st = pc.exact(case, k)[0] if L // k >= M else 2
            if st != 0:
                assert out["status"][f * nk + j] == lh.STATUS_INFEASIBLE, (what, case, k)
                continue
            assert out["status"][f * nk + j] == lh.STATUS_OPTIMAL, (what, case, k)
            assert pc.close(float(out["obj_by_k"][f * nk + j]), pc.objective(case, k)), (what, case, k)
        kb, ob = pc.best_k(case, [k for k in KS if L // k >= M])
        assert out["best_k"][f] == kb and pc.close(float(out["obj_value"][f]), ob), (what, case, int(out["best_k"][f]))
        if pc.unique(case, kb):
            xo = pc.exact(case, kb)[1]
            assert np.array_equal(out["w"][a:a + M], xo[:M]) and np.array_equal(out["n"][a:a + M], xo[M:2 * M]), (
                what, case)


def test_group_launch_over_pressured_tables(ctx):
    """Three resident M = 64 tables (the same seeds at memory scale 1, 1/16 and 1/64) rotated over 7 steps in
    one launch of the steps kernel, and the k-slot group launch on the two M = 16 tables: every table's
    outputs against the oracle's answers for that table."""
    import torch
    from fractions import Fraction

    from distilp_amd.solver.fleets import PlanGroup

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    for M, scales, persistent in ((64, (Fraction(1), pc.S16, pc.S64), True), (16, (pc.S16, pc.S64), True)):
        # (the k-slot group launch needs more than 64 fleets a table: the 16 seeds five times over)
        sets = [[(M, sc, s, "4bit") for s in range(16)] * (5 if M == 16 else 1) for sc in scales]
        tabs = [_resident(cs, 0.5, dev) for cs in sets]
        group = PlanGroup([dt for _, dt in tabs], ctx)
        assert group.persistent == persistent
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
        print(f"group launch M = {M}: kernels {sorted(ran)}")
        if M == 16:
            assert "halda_sweep_kslot_kernel" in ran, ran
        for cs, (table, dt) in zip(sets, tabs):
            check_resident(cs, table, dt, f"group M = {M} scale {cs[0][1]}")
        group.close()


# ------------------------------------------------------------------ contracts that inherit parity
def _as_oracle(r, case):
    """A HALDAResult of a case's fleet against the oracle's k-sweep."""
    M = case[0]
    kb, ob = pc.best_k(case, [k for k in KS if L // k >= M])
    assert r is not None and r.k == kb and pc.close(r.obj_value, ob), (case, r, kb, ob)
    if pc.unique(case, kb):
        xo = pc.exact(case, kb)[1]
        assert r.w == [int(v) for v in xo[:M]] and r.n == [int(v) for v in xo[M:2 * M]], (case, r)


def test_leave_one_out_under_pressure():
    """halda_leave_one_out_batch on four M = 64 and four M = 16 pressured fleets equals halda_solve_batch of
    the materialised lists (pydantic ==: k, w, n, sets and obj_value's bits); the first list of each size is
    also checked against the exact oracle directly."""
    model = pc.our_model()
    for M, scale in ((64, pc.S64), (16, pc.S16)):
        fleets = [pc.devices(s, M, scale) for s in range(4)]
        got = halda_leave_one_out_batch(fleets, model, kv_bits="4bit")
        for devs, row in zip(fleets, got):
            want = halda_solve_batch([devs[:i] + devs[i + 1:] for i in range(M)], model, kv_bits="4bit")
            assert row == want, M
        r, sub = got[0][0], fleets[0][1:]
        want, per_k = mo.halda_solve_oracle(sub, model, mip_gap=1e-4, kv_bits="4bit", solver="exact")
        assert r is not None and r.k == want["k"] and pc.close(r.obj_value, want["obj_value"]), (M, r, want)
        rec = next(q for q in per_k if q["k"] == want["k"])
        if rec["margin"] > 1e-7 * max(1.0, abs(rec["obj_value"])):
            assert (r.w, r.n) == (want["w"], want["n"]), (M, r, want)


@pytest.mark.parametrize("name,route", [("register", "fused"), ("kslot", "loop"), ("m5", "fused")])
def test_variants_under_pressure(name, route):
    """halda_solve_variants over kv 4bit / 8bit / fp16 equals one halda_solve_fleets call per variant, bit for
    bit (tests/test_gpu_variants.py's check_variants, which asserts the route), on the M = 64 batch (register
    route), the M = 16 batch (k-slot shape: the per-variant loop) and one M = 5 fleet (table route); the
    Python entry's first fleet is also checked against the oracle for the 4bit and fp16 variants."""
    from .test_gpu_variants import check_variants, solve_variants_device

    model = pc.our_model()
    cases = {"register": batch((64,)), "kslot": kslot_batch(), "m5": batch((5,), seeds=[1])}[name]
    fleets = [devs_of(c) for c in cases]
    variants = [(model, "4bit"), (model, "8bit"), (model, "fp16")]
    took = solve_variants_device(fleet_table(fleets, model), variants, KS)["route"]
    print(f"variants {name}: route {took}")
    assert took == route, (name, took)
    check_variants(fleets, variants, paths=((0, route),))
    got = halda_solve_variants(fleets[:1], variants)
    for (_, kv), row in zip(variants, got):
        _as_oracle(row[0], cases[0][:3] + (kv,))


# ------------------------------------------------------------------ plans
def test_plans_on_the_gpu_equal_the_numpy_specification():
    """halda_evaluate_plans_batch on the oracle's optima and their neighbours (pc.neighbour_plans, the
    slack_over_bound rejections of pc.NEIGHBOUR_EXTRA among them): status, objective within 1e-9, reason,
    bottleneck and cycle_time equal to evaluate_plan_np (tests/test_gpu_plans.py's _check_against_np); the
    optima must be feasible at the oracle's objective."""
    from .test_gpu_plans import _check_against_np

    model = pc.our_model()
    tabs, cases, slack = {}, [], 0
    for case, k, kind, w, n in pc.neighbour_plans():
        if case not in tabs:
            tabs[case] = fleet_table([devs_of(case)], model)
        if kind == "optimum":
            ok, obj = True, pc.objective(case, k)
        else:
            e = pl.evaluate_plan_np(tabs[case], model, 0, k, w, n, 0.5)
            ok, obj = e.feasible, e.obj_value
            slack += bool(e.reason & pl.REASON_SLACK)
        cases.append((case, devs_of(case), k, w, n, ok, obj))
    assert slack >= 1 and len(cases) >= 2500
    _check_against_np(cases, model)


@pytest.mark.parametrize("path,name,route", [(0, "register", "two_launch"), (2, "register", "fused"),
                                             (0, "kslot", "two_launch"), (2, "kslot", None)])
def test_sweep_with_incumbents_on_both_plan_paths(ctx, path, name, route):
    """halda_solve_fleets_plans (the sweep and the incumbents' evaluation in one call) on the default path and
    on halda_set_plans_path(ctx, 2): the sweep against the oracle, the evaluation of each fleet's first
    neighbour plan against evaluate_plan_np; and the sweep's own (best_k, w, n) evaluates to its obj_value --
    bit for bit against the one-fleet-per-wave sweep, as tests/test_gpu_plans.py holds it."""
    model = pc.our_model()
    cases = SWEEPS[name][0]()
    table = fleet_table([devs_of(c) for c in cases], model)
    first = {}
    for case, k, kind, w, n in pc.neighbour_plans():
        if kind != "optimum" and k == 1:
            first.setdefault(case, (k, w, n))
    k, w, n = pl._plan_arrays(table, [first[c] for c in cases], allow_none=False)
    pl.set_plans_path(ctx, path)
    try:
        res, buf = pl.solve_plans_table(table, model, KS, k, w, n, 0.5)
        got_route = pl.last_plans_route(ctx)
    finally:
        pl.set_plans_path(ctx, 0)
    print(f"{name} path {path}: route {got_route}")
    assert got_route in ("fused", "two_launch") and (route is None or got_route == route), got_route
    nk = len(KS)
    for f, case in enumerate(cases):
        M, a = case[0], int(table.dev_off[f])
        e = pl.evaluate_plan_np(table, model, f, *first[case], 0.5)
        assert (buf.status[f], buf.reason[f], buf.bottleneck[f]) == (e.status, e.reason, e.bottleneck), (case, e)
        if e.feasible:
            assert buf.cycle[f] == e.cycle and pc.close(float(buf.obj[f]), e.obj_value), case
        for j, kk in enumerate(KS):
            off = int(res.x_off[f * nk + j])
            if L // kk < M:
                assert off == -1 and res.status[f, j] == lh.STATUS_INFEASIBLE
                continue
            assert res.status[f, j] == lh.STATUS_OPTIMAL, (case, kk)
            pc.check_x(res.x[off:off + 7 * M + 1], case, kk, f"plans path {path}")
        kb, ob = pc.best_k(case, [q for q in KS if L // q >= M])
        assert res.best_k[f] == kb and pc.close(float(res.obj_value[f]), ob), case
    ctx.set_fleets_path("wave")
    try:
        wave = solve_table(table, model, KS, 0.5)
    finally:
        ctx.set_fleets_path("fused")
    own = pl.evaluate_table(table, model, wave.best_k, wave.w, wave.n, 0.5)
    assert (own.status == lh.STATUS_OPTIMAL).all() and (own.reason == 0).all()
    assert np.array_equal(own.obj, wave.obj_value)  # bit for bit
    assert np.array_equal(wave.best_k, res.best_k) and np.array_equal(wave.w, res.w) and np.array_equal(wave.n, res.n)
    assert np.allclose(own.obj, res.obj_value, rtol=1e-12, atol=0.0)


# ------------------------------------------------------------------ bounds
@pytest.mark.parametrize("M,k,route", [(64, 1, "fused"), (16, 1, "general"), (16, 2, "general"),
                                       (16, 4, "general")])
def test_bounded_sweep_under_pressure(ctx, M, k, route):
    """halda_solve_bounded_batch on the pressured fleets within the D = 2 move box of tests/bounds_cases.py
    around the pressured optimum of seed + 100, and within the uniform cap: against the exact oracle on the
    dense problem with the w columns' bounds narrowed. An empty box must come back infeasible; at least half
    of the cases are feasible."""
    model = pc.our_model()
    W = L // k
    cases = batch((M,))
    fleets, boxes, kinds = [], [], []
    for case in cases:
        inc = (M, case[1], case[2] + 100, "4bit")
        st, x0, _, _ = pc.exact(inc, k)
        assert st == 0
        w0 = [int(v) for v in x0[:M]]
        for kind, box in ((2, ([max(1, v - 2) for v in w0], [min(W, v + 2) for v in w0])),
                          ("cap", ([1] * M, [min(W, -(-W // M) + 1)] * M))):
            fleets.append(devs_of(case))
            boxes.append(box)
            kinds.append((case, kind))
    got = bd.halda_solve_bounded_batch(fleets, model, boxes, k_candidates=[k], kv_bits="4bit")
    assert bd.last_bounds_route(ctx) == route, bd.last_bounds_route(ctx)
    feasible = 0
    for (case, kind), (lo, hi), r in zip(kinds, boxes, got):
        p = dict(pc.problem(case, k))
        p["lb"], p["ub"] = p["lb"].copy(), p["ub"].copy()
        p["lb"][:M], p["ub"][:M] = lo, hi
        st, xo, b1, b2, _ = mo.exact_solve(p)
        if st != 0:
            assert st == 2 and r is None, (case, kind, r)
            continue
        feasible += 1
        assert r is not None and r.k == k, (case, kind)
        assert pc.close(r.obj_value, mo.objective_value(p, xo)), (case, kind, r.obj_value, mo.objective_value(p, xo))
        assert all(a <= v <= b for a, v, b in zip(lo, r.w, hi)), (case, kind)
        if mo.uniqueness_margin_ok(b1, b2):
            assert r.w == [int(v) for v in xo[:M]] and r.n == [int(v) for v in xo[M:2 * M]], (case, kind, r)
    print(f"bounded M = {M} k = {k}: {feasible} of {len(got)} feasible")
    assert feasible >= 0.5 * len(got), (feasible, len(got))


# ------------------------------------------------------------------ the reference's recorded results
def test_python_entries_match_the_recorded_pressure_results():
    """halda_solve and halda_solve_batch on the fleets of tests/golden/pressure.json against the reference's
    recorded HALDAResult, under the standing rule (tests/pressure_cases.py result_mismatch)."""
    import contextlib
    import io

    model = pc.our_model()
    recs = load_json("pressure.json")["fleets"]
    fleets = [pc.golden_devices(r) for r in recs]
    got = halda_solve_batch(fleets, model, mip_gap=1e-4, kv_bits="4bit")
    for rec, devs, r in zip(recs, fleets, got):
        _, per_k = mo.halda_solve_oracle(devs, model, mip_gap=1e-4, kv_bits="4bit", solver="exact")
        assert pc.result_mismatch(r, rec, per_k) is None, (rec["M"], rec["scale"], rec["seed"],
                                                            pc.result_mismatch(r, rec, per_k))
        if rec["seed"] == 0:
            with contextlib.redirect_stdout(io.StringIO()):
                one = halda_solve(devs, model, mip_gap=1e-4, plot=False, kv_bits="4bit")
            assert pc.result_mismatch(one, rec, per_k) is None, (rec["M"], rec["scale"])
