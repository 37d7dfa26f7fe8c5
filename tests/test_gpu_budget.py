"""The total move budget on the GPU (halda_sweep_budget_kernel) against tests/golden/budget.json: every case of
both lists, the edge shapes, batch = single, a resident table, two streams, and the kernel's code object."""

import math

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import budget as bg
from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import DeviceFleetTable, fleet_table

from . import bounds_cases as bc
from . import budget_cases as bu
from .test_abi import kernel_resources

pytestmark = pytest.mark.gpu

KVB = "4bit"  # kv factor 0.5, bounds_cases.KV


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


def check_point(model, devs, k, w0, p, pt, want, lo=None, hi=None, tag=None):
    """One frontier point against the oracle's objective (None: infeasible) and its own constraints."""
    if want is None:
        assert pt.plan is None and pt.obj_value == math.inf and pt.moved_layers == 0, (tag, p, pt)
        return
    assert pt.plan is not None, (tag, p)
    assert pt.budget_layers == 2 * p and pt.plan.k == k and pt.plan.obj_value == pt.obj_value
    assert bc.rel(pt.obj_value, want) <= 1e-9, (tag, p, pt.obj_value, want)
    w, n, W = pt.plan.w, pt.plan.n, int(model.L) // k
    assert sum(w) == W and all(1 <= a <= W for a in w) and all(0 <= b <= a for a, b in zip(w, n)), (tag, p, w, n)
    if lo is not None:
        assert all(a >= b for a, b in zip(w, lo)), (tag, p)
    if hi is not None:
        assert all(a <= b for a, b in zip(w, hi)), (tag, p)
    assert sum(max(0, a - b) for a, b in zip(w, w0)) <= p, (tag, p, w, w0)
    assert pt.moved_layers == sum(abs(a - b) for a, b in zip(w, w0)) <= 2 * p, (tag, p)


def check_frontier_prices(model, fleets, frontiers, tag):
    """Every returned plan priced by halda_evaluate_plan equals its point's objective bit for bit (one call);
    the frontier is non-increasing."""
    devs, plans, objs = [], [], []
    for f, fr in zip(fleets, frontiers):
        last = math.inf
        for pt in fr:
            assert pt.obj_value <= last, (tag, pt)
            last = pt.obj_value
            if pt.plan is not None:
                devs.append(f)
                plans.append((pt.plan.k, pt.plan.w, pt.plan.n))
                objs.append(pt.obj_value)
    if plans:
        ev = pl.halda_evaluate_plans_batch(devs, model, plans, KVB)
        for e, o, p in zip(ev, objs, plans):
            assert e.feasible and e.obj_value == o, (tag, p, e.obj_value, o)


# ------------------------------------------------------------------ 1. both case lists
@pytest.fixture(scope="module")
def solved(llama_online_model):
    """Both lists solved once: {(M, k, s): frontier}; one GPU call per (list, k)."""
    model, out = llama_online_model, {}
    for cases, P in ((bu.LIST_A, max(bu.PS_A)), (bu.LIST_B, max(bu.PS_B))):
        gold = bu.golden()["A" if cases is bu.LIST_A else "B"]
        fleets = [list(bc.devices(M, s)) for M, k, s in cases]
        incs = [(k, gold[bu.key(M, k, s)]["w0"], [0] * M) for M, k, s in cases]
        got = bg.halda_move_frontier_batch(fleets, model, incs, 2 * P, KVB)
        for c, fr in zip(cases, got):
            out[c] = fr
    return out


@pytest.mark.parametrize("name", ["A", "B"])
def test_every_list_case_equals_the_oracle(llama_online_model, solved, name):
    model = llama_online_model
    cases, ps = (bu.LIST_A, bu.PS_A) if name == "A" else (bu.LIST_B, bu.PS_B)
    gold = bu.golden()[name]
    for M, k, s in cases:
        g, fr = gold[bu.key(M, k, s)], solved[(M, k, s)]
        assert len(fr) == max(ps) + 1
        for p in ps:
            check_point(model, None, k, g["w0"], p, fr[p], g["obj"][str(p)], tag=(M, k, s))
        for p, pt in enumerate(fr):  # the points without a recorded answer keep their own constraints
            check_point(model, None, k, g["w0"], p, pt, pt.obj_value if pt.plan else None, tag=(M, k, s))
    check_frontier_prices(model, [list(bc.devices(M, s)) for M, k, s in cases], [solved[c] for c in cases], name)


# The cases whose free optimum moves more layers than the gate admits for their fleet width (P <= 63 and the
# 160 KiB slice: P <= 63 on 3 devices, 62 on 4, 55 on 8 and 47 on 16 at k = 1): {case: free_p}, by the exact
# oracle (tests/golden/budget.json "free_p"). No launch can reach them; every other case of both lists is checked.
BEYOND_THE_GATE = {
    "A": {(3, 1, 2): 77, (3, 1, 3): 69, (4, 1, 0): 73, (4, 1, 2): 76},
    "B": {(8, 1, 0): 72, (8, 1, 1): 61, (8, 1, 2): 72, (8, 1, 3): 59, (8, 1, 5): 63,
          (16, 1, 0): 64, (16, 1, 1): 53, (16, 1, 2): 64, (16, 1, 4): 64, (16, 1, 5): 64},
}


def gate_p(M, k):
    """The largest P the launch's gate admits for fleets of M devices at k."""
    return max(P for P in range(bg.MAX_P + 1) if bg.budget_lds_bytes(M, P, k) <= bg.LDS_BUDGET)


@pytest.mark.parametrize("name", ["A", "B"])
def test_ends_of_the_frontier_equal_the_bounded_solves(llama_online_model, solved, name):
    """Point 0 is "w pinned, n re-optimised"; the point at the free optimum's own move count, and every later
    one, is the free optimum at that k (1e-12: DESIGN.md section 4.5's cross-path bound). Each (M, k) group runs
    at the least P that reaches every one of its cases, or at the largest its gate admits."""
    model = llama_online_model
    cases = bu.LIST_A if name == "A" else bu.LIST_B
    gold = bu.golden()[name]
    beyond, reached = {}, 0
    for M, k in sorted({c[:2] for c in cases}):
        sub = [c for c in cases if c[:2] == (M, k)]
        P = min(gate_p(M, k), max(gold[bu.key(*c)]["free_p"] for c in sub))
        fleets = [list(bc.devices(M, s)) for _, _, s in sub]
        w0s = [gold[bu.key(*c)]["w0"] for c in sub]
        pinned = bd.halda_solve_bounded_batch(fleets, model, [(w0, w0) for w0 in w0s], [k], KVB)
        free = bd.halda_solve_bounded_batch(fleets, model, [None] * len(sub), [k], KVB)
        wide = bg.halda_move_frontier_batch(fleets, model, [(k, w0, [0] * M) for w0 in w0s], 2 * P, KVB)
        for c, w0, a, b, fw in zip(sub, w0s, pinned, free, wide):
            fr = solved[c]
            assert a is not None and bc.rel(fr[0].obj_value, a.obj_value) <= 1e-12, (c, fr[0].obj_value, a.obj_value)
            assert fr[0].plan.w == list(w0) and fr[0].moved_layers == 0
            n = min(len(fr), len(fw))
            assert [pt.obj_value for pt in fw[:n]] == [pt.obj_value for pt in fr[:n]], c  # another P: same points
            ps = sum(max(0, x - y) for x, y in zip(b.w, w0))
            assert ps == gold[bu.key(*c)]["free_p"], (c, ps)
            assert all(pt.obj_value >= b.obj_value - 1e-12 * max(1.0, abs(b.obj_value)) for pt in fw), c
            if ps > P:
                beyond[c] = ps
                continue
            reached += 1
            assert bc.rel(fw[ps].obj_value, b.obj_value) <= 1e-12, (c, ps, fw[ps].obj_value, b.obj_value)
            assert all(pt.obj_value == fw[ps].obj_value for pt in fw[ps:]), c
            if ps:
                assert fw[ps - 1].obj_value > fw[ps].obj_value, c  # unique optimum: one layer fewer is worse
    assert beyond == BEYOND_THE_GATE[name] and reached == len(cases) - len(beyond)


# ------------------------------------------------------------------ 1b. the kernel's own outputs
def check_raw(model, fleets, k, w0s, P, los=None, his=None, tag=None):
    """The raw halda_frontier of one call: on OPTIMAL points obj is halda_eval_plans' device-formed objective of
    the returned (k, w, n) bit for bit and moved = sum |w - w0|; elsewhere obj = +inf, moved = 0 and the
    plan's planes are zero. Returns the FrontierSolve."""
    table = fleet_table(fleets, model)
    w0 = np.concatenate([np.asarray(w, np.int32) for w in w0s])
    lo = None if los is None else bg._flat(table, los, 0)
    hi = None if his is None else bg._flat(table, his, bg.INT32_MAX)
    res = bg.solve_budget_table(table, model, k, w0, P, bc.KV, lo, hi)
    karr = np.full(table.n_fleets, k, np.int32)
    off = table.dev_off
    for p in range(P + 1):
        buf = pl.evaluate_table(table, model, karr, res.w[p], res.n[p], bc.KV)
        for f in range(table.n_fleets):
            a, b = int(off[f]), int(off[f + 1])
            if res.status[f, p] == lh.STATUS_OPTIMAL:
                assert buf.status[f] == lh.STATUS_OPTIMAL and res.obj[f, p] == buf.obj[f], (tag, f, p, res.obj[f, p],
                                                                                          buf.obj[f])
                assert res.moved[f, p] == np.abs(res.w[p, a:b] - w0[a:b]).sum(), (tag, f, p)
            else:
                assert res.status[f, p] == lh.STATUS_INFEASIBLE, (tag, f, p)
                assert res.obj[f, p] == math.inf and res.moved[f, p] == 0, (tag, f, p)
                assert not res.w[p, a:b].any() and not res.n[p, a:b].any(), (tag, f, p)
    return res


@pytest.mark.parametrize("name", ["A", "B"])
def test_kernel_objective_is_the_plan_evaluation_bit_for_bit(llama_online_model, solved, name):
    """Every list case, one call per k: the kernel's obj against halda_eval_plans on its own plan, and the
    Python frontier carries exactly the kernel's plans."""
    model = llama_online_model
    cases, ps = (bu.LIST_A, bu.PS_A) if name == "A" else (bu.LIST_B, bu.PS_B)
    gold = bu.golden()[name]
    for k in sorted({c[1] for c in cases}):
        sub = [c for c in cases if c[1] == k]
        res = check_raw(model, [list(bc.devices(M, s)) for M, _, s in sub], k, [gold[bu.key(*c)]["w0"] for c in sub],
                        max(ps), tag=(name, k))
        assert (res.status == lh.STATUS_OPTIMAL).all()
        assert (np.diff(res.obj, axis=1) <= 0).all()  # the device-formed frontier is non-increasing
        a = 0
        for f, c in enumerate(sub):
            for p in ps:
                assert bc.rel(res.obj[f, p], gold[bu.key(*c)]["obj"][str(p)]) <= 1e-9, (c, p)
                assert solved[c][p].plan.w == res.w[p, a:a + c[0]].tolist(), (c, p)
            a += c[0]


@pytest.mark.parametrize("name", ["one_device", "wide_64", "cap_excludes_w0", "crossing_box", "clipped_window",
                                  "tied_k2", "pressured", "pressured_cap_excludes_w0", "pressured_w_min"])
def test_kernel_outputs_on_the_edge_shapes(llama_online_model, name):
    model = llama_online_model
    e, g = bu.edge_cases(model)[name], bu.golden()["edge"][name]["obj"]
    res = check_raw(model, [e["devs"]], e["k"], [e["w0"]], e["P"], None if e["w_min"] is None else [e["w_min"]],
                    None if e["w_max"] is None else [e["w_max"]], tag=name)
    for p in range(e["P"] + 1):
        if g[str(p)] is None:
            assert res.status[0, p] == lh.STATUS_INFEASIBLE, (name, p)
        else:
            assert res.status[0, p] == lh.STATUS_OPTIMAL and bc.rel(res.obj[0, p], g[str(p)]) <= 1e-9, (name, p)


# ------------------------------------------------------------------ 1c. list P: memory-pressured fleets
def p_groups():
    """List P by launch: {(M, scale): cases}; one budget (the largest recorded p) per group."""
    out = {}
    for c in bu.LIST_P:
        out.setdefault(c[:2], []).append(c)
    return out


@pytest.fixture(scope="module")
def solved_p(llama_online_model):
    """List P solved once: {case: frontier}; one Python call per (M, scale), one GPU call per k inside it."""
    from . import pressure_cases as pc

    model, gold, out = llama_online_model, bu.golden()["P"], {}
    for (M, sc), cases in p_groups().items():
        fleets = [pc.devices(s, M, sc) for _, _, _, s in cases]
        incs = [(k, gold[bu.key_p(*c)]["w0"], [0] * M) for c in cases for k in [c[2]]]
        got = bg.halda_move_frontier_batch(fleets, model, incs, 2 * max(bu.ps_of_p(M)), KVB)
        out.update(zip(cases, got))
    return out


def test_list_p_equals_the_oracle(llama_online_model, solved_p):
    """Every recorded point of the pressured list within 1e-9 of the golden, every point under its own
    constraints, the frontier non-increasing and every plan priced by halda_evaluate_plan bit for bit."""
    from . import pressure_cases as pc

    model, gold = llama_online_model, bu.golden()["P"]
    for c in bu.LIST_P:
        M, sc, k, s = c
        g, fr = gold[bu.key_p(*c)], solved_p[c]
        assert len(fr) == max(bu.ps_of_p(M)) + 1
        for p in bu.ps_of_p(M):
            check_point(model, None, k, g["w0"], p, fr[p], g["obj"][str(p)], tag=c)
        for p, pt in enumerate(fr):
            check_point(model, None, k, g["w0"], p, pt, pt.obj_value if pt.plan else None, tag=c)
    check_frontier_prices(model, [pc.devices(s, M, sc) for M, sc, _, s in bu.LIST_P], [solved_p[c] for c in bu.LIST_P],
                          "P")


def test_list_p_kernel_objective_is_the_plan_evaluation_bit_for_bit(llama_online_model, solved_p):
    """One raw call per (M, scale, k): the kernel's obj against halda_eval_plans on its own plan (check_raw), the
    device-formed frontier non-increasing, the recorded points within 1e-9, the Python frontier's plans the
    kernel's."""
    from . import pressure_cases as pc

    model, gold = llama_online_model, bu.golden()["P"]
    for (M, sc), cases in p_groups().items():
        for k in sorted({c[2] for c in cases}):
            sub = [c for c in cases if c[2] == k]
            res = check_raw(model, [pc.devices(c[3], M, sc) for c in sub], k, [gold[bu.key_p(*c)]["w0"] for c in sub],
                            max(bu.ps_of_p(M)), tag=("P", M, sc, k))
            assert (res.status == lh.STATUS_OPTIMAL).all()
            assert (np.diff(res.obj, axis=1) <= 0).all()
            for f, c in enumerate(sub):
                for p in bu.ps_of_p(M):
                    assert bc.rel(res.obj[f, p], gold[bu.key_p(*c)]["obj"][str(p)]) <= 1e-9, (c, p)
                    assert solved_p[c][p].plan.w == res.w[p, f * M:(f + 1) * M].tolist(), (c, p)


# list P's cases beyond the gate (gate_p: 60 / 59 on 5 devices, 47 / 45 on 16), by the exact oracle's free_p
def _beyond_p():
    from . import pressure_cases as pc

    return {(5, pc.S16, 1, 1): 64, (16, pc.S16, 1, 0): 49, (16, pc.S64, 1, 0): 64, (16, pc.S64, 1, 1): 61}


def test_list_p_ends_of_the_frontier_equal_the_bounded_solves(llama_online_model, solved_p):
    """Point 0 equals halda_solve_bounded with w pinned (1e-12); the point at the free optimum's own move count,
    and every later one, equals the free optimum at that k wherever the gate reaches it; elsewhere no point
    beats it."""
    from . import pressure_cases as pc

    model, gold = llama_online_model, bu.golden()["P"]
    beyond, reached = {}, 0
    for (M, sc), cases in p_groups().items():
        for k in sorted({c[2] for c in cases}):
            sub = [c for c in cases if c[2] == k]
            P = min(gate_p(M, k), max(gold[bu.key_p(*c)]["free_p"] for c in sub))
            fleets = [pc.devices(c[3], M, sc) for c in sub]
            w0s = [gold[bu.key_p(*c)]["w0"] for c in sub]
            pinned = bd.halda_solve_bounded_batch(fleets, model, [(w0, w0) for w0 in w0s], [k], KVB)
            free = bd.halda_solve_bounded_batch(fleets, model, [None] * len(sub), [k], KVB)
            wide = bg.halda_move_frontier_batch(fleets, model, [(k, w0, [0] * M) for w0 in w0s], 2 * P, KVB)
            for c, w0, a, b, fw in zip(sub, w0s, pinned, free, wide):
                fr = solved_p[c]
                assert a is not None and bc.rel(fr[0].obj_value, a.obj_value) <= 1e-12, (c, fr[0].obj_value, a.obj_value)
                assert fr[0].plan.w == list(w0) and fr[0].moved_layers == 0
                n = min(len(fr), len(fw))
                assert [pt.obj_value for pt in fw[:n]] == [pt.obj_value for pt in fr[:n]], c
                ps = sum(max(0, x - y) for x, y in zip(b.w, w0))
                assert ps == gold[bu.key_p(*c)]["free_p"], (c, ps)
                assert all(pt.obj_value >= b.obj_value - 1e-12 * max(1.0, abs(b.obj_value)) for pt in fw), c
                if ps > P:
                    beyond[c] = ps
                    continue
                reached += 1
                assert bc.rel(fw[ps].obj_value, b.obj_value) <= 1e-12, (c, ps, fw[ps].obj_value, b.obj_value)
                assert all(pt.obj_value == fw[ps].obj_value for pt in fw[ps:]), c
                if ps:
                    assert fw[ps - 1].obj_value > fw[ps].obj_value, c
    assert beyond == _beyond_p() and reached == len(bu.LIST_P) - len(beyond)


# ------------------------------------------------------------------ 2. the edge shapes
@pytest.mark.parametrize("name", ["one_device", "wide_64", "cap_excludes_w0", "crossing_box", "clipped_window",
                                  "tied_k2", "pressured", "pressured_cap_excludes_w0", "pressured_w_min"])
def test_edge_shape(llama_online_model, name):
    model = llama_online_model
    e, g = bu.edge_cases(model)[name], bu.golden()["edge"][name]["obj"]
    fr = bg.halda_move_frontier(e["devs"], model, (e["k"], e["w0"], [0] * len(e["w0"])), 2 * e["P"], KVB,
                                w_min=e["w_min"], w_max=e["w_max"])
    assert len(fr) == e["P"] + 1
    for p, pt in enumerate(fr):
        check_point(model, e["devs"], e["k"], e["w0"], p, pt, g[str(p)], e["w_min"], e["w_max"], tag=name)
    check_frontier_prices(model, [e["devs"]], [fr], name)
    if name == "clipped_window":  # the window really is clipped at w = 1 and at w = W
        assert e["w0"][0] - e["P"] < 1 and e["w0"][2] + e["P"] > int(model.L) // e["k"]
    if name == "pressured_cap_excludes_w0":
        assert [pt.plan is None for pt in fr] == [True, True, False, False]
        assert all(a <= b for pt in fr[2:] for a, b in zip(pt.plan.w, e["w_max"]))
    if name == "pressured_w_min":
        assert [pt.plan is None for pt in fr] == [True, False, False, False]
        assert all(a >= b for pt in fr[1:] for a, b in zip(pt.plan.w, e["w_min"]))
    if name == "cap_excludes_w0":
        assert [pt.plan is None for pt in fr] == [True, True, False, False]
        with pytest.raises(RuntimeError):
            bg.halda_solve_budget(e["devs"], model, (e["k"], e["w0"], [0] * 4), 2, KVB, w_max=e["w_max"])
        r = bg.halda_solve_budget(e["devs"], model, (e["k"], e["w0"], [0] * 4), 6, KVB, w_max=e["w_max"])
        assert r.w == fr[-1].plan.w and r.obj_value == fr[-1].obj_value


def test_zero_budget_and_a_budget_beyond_any_useful_move(llama_online_model):
    model = llama_online_model
    M, k, s = 4, 2, 0
    devs, g = list(bc.devices(M, s)), bu.golden()["A"][bu.key(M, k, s)]
    inc = (k, g["w0"], [0] * M)
    for B in (0, 1):  # P = 0: one point, w pinned
        fr = bg.halda_move_frontier(devs, model, inc, B, KVB)
        assert len(fr) == 1 and fr[0].plan.w == g["w0"] and fr[0].moved_layers == 0
        assert bc.rel(fr[0].obj_value, g["obj"]["0"]) <= 1e-9
    free = bd.halda_solve_bounded(devs, model, k_candidates=[k], kv_bits=KVB)
    ps = sum(max(0, a - b) for a, b in zip(free.w, g["w0"]))
    P = ps + 6
    fr = bg.halda_move_frontier(devs, model, inc, 2 * P, KVB)
    assert len(fr) == P + 1 and bc.rel(fr[ps].obj_value, free.obj_value) <= 1e-12
    assert all(pt.obj_value == fr[ps].obj_value and pt.plan.w == fr[ps].plan.w and pt.moved_layers <= 2 * ps
               for pt in fr[ps:])
    if ps:
        assert fr[ps - 1].obj_value > fr[ps].obj_value
    for p in bu.PS_A:
        assert bc.rel(fr[p].obj_value, g["obj"][str(p)]) <= 1e-9, p  # a larger P changes no earlier point


# ------------------------------------------------------------------ 3. batch = single, mixed sizes
def test_a_mixed_batch_equals_the_single_calls_bit_for_bit(llama_online_model):
    model, k, P = llama_online_model, 2, 3
    gold = bu.golden()
    cases = [(3, k, 0), (8, k, 1), (16, k, 2), (4, k, 3)]
    fleets = [list(bc.devices(M, s)) for M, _, s in cases]
    incs = [(k, gold["A" if M < 8 else "B"][bu.key(M, k, s)]["w0"], [0] * M) for M, _, s in cases]
    batch = bg.halda_move_frontier_batch(fleets, model, incs, 2 * P, KVB)
    for c, devs, inc, fr in zip(cases, fleets, incs, batch):
        one = bg.halda_move_frontier(devs, model, inc, 2 * P, KVB)
        assert one == fr, c
        g = gold["A" if c[0] < 8 else "B"][bu.key(*c)]["obj"]
        for p in (0, 1, 2):
            assert bc.rel(fr[p].obj_value, g[str(p)]) <= 1e-9, (c, p)


# ------------------------------------------------------------------ 4. a resident table, two streams
def _resident(model, seeds, k, P):
    torch, dev = _torch()
    gold = bu.golden()["B"]
    fleets = [list(bc.devices(16, s)) for s in seeds]
    table = fleet_table(fleets, model)
    w0 = np.concatenate([np.asarray(gold[bu.key(16, k, s)]["w0"], np.int32) for s in seeds])
    dt = DeviceFleetTable(table, model, [k], bc.KV, dev)
    dt.set_budget(k, w0, P)
    return dt, table, w0


def test_launch_with_budget_equals_the_one_shot_call(llama_online_model):
    torch, dev = _torch()
    model, k, P = llama_online_model, 2, 4
    ctx = lh.get_context(0)
    dt, table, w0 = _resident(model, (0, 1, 2), k, P)
    want = bg.solve_budget_table(table, model, k, w0, P, bc.KV)
    for bad_p in (64, 48, -1):  # beyond 63, beyond the LDS budget on 16 devices, negative: the Python gate
        with pytest.raises(ValueError):
            dt.set_budget(k, w0, bad_p)
    dt.set_budget(k, w0, P)
    s = torch.cuda.Stream(dev)
    dt.launch_with_budget(ctx, s.cuda_stream)
    torch.cuda.synchronize(dev)
    for f in ("status", "obj", "moved", "w", "n"):
        assert np.array_equal(dt.budget_out[f].cpu().numpy(), getattr(want, f)), f
    assert (want.status == lh.STATUS_OPTIMAL).all()
    # the kernel's own objective is halda_eval_plans' device-formed one of the same plan, bit for bit
    for p in range(P + 1):
        buf = pl.evaluate_table(table, model, np.full(table.n_fleets, k, np.int32), want.w[p], want.n[p], bc.KV)
        assert np.array_equal(buf.obj, want.obj[:, p]), p
    # in place: the incumbents become point P's plans; the new point 0 prices exactly them
    with torch.cuda.stream(s):
        dt.budget_w0.copy_(dt.budget_out["w"][P])
    dt.launch_with_budget(ctx, s.cuda_stream)
    torch.cuda.synchronize(dev)
    got = {f: dt.budget_out[f].cpu().numpy() for f in ("status", "obj", "moved", "w")}
    assert np.array_equal(got["w"][0], want.w[P]) and (got["moved"][:, 0] == 0).all()
    assert np.allclose(got["obj"][:, 0], want.obj[:, P], rtol=1e-12, atol=0.0)


def test_launches_on_two_streams_give_the_synchronous_answers(llama_online_model):
    torch, dev = _torch()
    model, P = llama_online_model, 4
    ctx = lh.get_context(0)
    tabs, want = [], []
    for seeds, k in (((0, 1, 2), 1), ((3, 4, 5), 2)):
        dt, table, w0 = _resident(model, seeds, k, P)
        dt.launch_with_budget(ctx, 0)
        torch.cuda.synchronize(dev)
        want.append({f: v.cpu().numpy().copy() for f, v in dt.budget_out.items()})
        tabs.append(dt)
    for dt in tabs:
        for v in dt.budget_out.values():
            v.fill_(-7)
    torch.cuda.synchronize(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for _ in range(3):
        for dt, s in zip(tabs, streams):
            dt.launch_with_budget(ctx, s.cuda_stream)
    torch.cuda.synchronize(dev)
    for dt, w in zip(tabs, want):
        for f, v in dt.budget_out.items():
            assert np.array_equal(v.cpu().numpy(), w[f]), f


# ------------------------------------------------------------------ 5. the C entries' gate and the code object
def test_c_entry_rejects_what_is_outside_the_gate(llama_online_model):
    import ctypes

    from distilp_amd.solver.fleets import HaldaBudgetC, HaldaFrontierC, _host_struct, model_struct

    model = llama_online_model
    ctx = lh.get_context(0)
    lib = ctx.lib
    table = fleet_table([list(bc.devices(4, 0))], model)
    fs, keep = _host_struct(table)
    m = model_struct(model, bc.KV)
    W = int(model.L)
    P1 = 64
    st, obj = np.zeros(P1, np.int32), np.zeros(P1)
    mv, w, n = np.zeros(P1, np.int32), np.zeros(P1 * 4, np.int32), np.zeros(P1 * 4, np.int32)
    fr = HaldaFrontierC(4, st.ctypes.data, obj.ctypes.data, mv.ctypes.data, w.ctypes.data, n.ctypes.data)

    def call(w0, max_p, k=1):
        a = np.asarray(w0, np.int32)
        b = HaldaBudgetC(a.ctypes.data, None, None, max_p)
        with ctx._lock:
            return lib.halda_solve_fleets_budget_host(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), k, ctypes.byref(b),
                                                      ctypes.byref(fr))

    assert call([W - 3, 1, 1, 1], 2) == 0 and st[0] == lh.STATUS_OPTIMAL
    assert call([W - 4, 1, 1, 1], 2) == -22 and "sum w0" in lh.last_error(lib)  # sum w0 != W
    assert call([W - 2, 0, 1, 1], 2) == -22  # w0_i < 1
    assert call([W - 3, 1, 1, 1], 64) == -22 and "max_p" in lh.last_error(lib)
    assert call([W - 3, 1, 1, 1], 63) == -22 and "LDS" in lh.last_error(lib)
    assert call([W - 3, 1, 1, 1], -1) == -22
    assert call([W - 3, 1, 1, 1], 2, k=0) == -22
    del keep


def test_budget_kernel_code_object(tmp_path):
    """No spilled VGPR, no scratch, and within the VGPR budget of the two waves per SIMD its __launch_bounds__
    names (256)."""
    r = kernel_resources(tmp_path)["halda_sweep_budget_kernel"]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 256, r
