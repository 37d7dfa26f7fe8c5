"""The change frontier on the GPU (halda_sweep_change_kernel) against tests/golden/change.json: every case of every
list, the edge shapes, the identities with the budget kernel, the materialised lists and the plan evaluation, the
far end against the free re-solve, the C gate, a resident table and the CLI lines."""

import ctypes
import math

import numpy as np
import pytest

from distilp_amd.cli import solver as cli
from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import budget as bg
from distilp_amd.solver import change as ch
from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import DeviceFleetTable, fleet_table
from distilp_amd.solver.subfleets import halda_solve_subfleets, pack_items

from . import bounds_cases as bc
from . import budget_cases as bu
from . import change_cases as cc
from .test_abi import kernel_resources

pytestmark = pytest.mark.gpu

KVB = "4bit"  # kv factor 0.5, bounds_cases.KV


def lists_of(model):
    """{name: [(golden key, parent devs, kept indices, k, w0, ps)]} of every list case, every device lost in turn."""
    out = {n: [] for n in ("A", "B", "W", "S", "P")}
    for name, cases in (("A", cc.LIST_A), ("B", cc.LIST_B), ("W", [cc.WIDE]), ("S", cc.LIST_S)):
        for M, k, s in cases:
            devs, w = cc.stale_parent(model, M, k, s) if name == "S" else cc.parent(model, M, k, s)
            ps = cc.PS_A if name == "S" else cc.ps_of(M)
            for lost in range(M):
                keep, _, w0 = cc.lose(devs, w, lost)
                out[name].append((cc.key(M, k, s, lost), devs, keep, k, w0, ps))
    for M, sc, k, s in cc.LIST_P:
        devs, w = cc.parent(model, M, k, s, sc)
        for lost in range(M):
            keep, _, w0 = cc.lose(devs, w, lost)
            out["P"].append((cc.key_p(M, sc, k, s, lost), devs, keep, k, w0, cc.ps_of(M)))
    return out


def solve_cases(model, cases, P=None):
    """One halda_change_frontiers call per k over `cases` (lists_of entries): parents packed once each, lists of
    mixed lengths in one launch. {golden key: frontier}."""
    out = {}
    for k in sorted({c[3] for c in cases}):
        sub = [c for c in cases if c[3] == k]
        parents, at = [], {}
        for c in sub:
            if id(c[1]) not in at:
                at[id(c[1])] = len(parents)
                parents.append(c[1])
        got = ch.halda_change_frontiers(parents, model, [(at[id(c[1])], c[2]) for c in sub], k, [c[4] for c in sub],
                                        max(max(c[5]) for c in sub) if P is None else P, KVB)
        out.update({c[0]: fr for c, fr in zip(sub, got)})
    return out


@pytest.fixture(scope="module")
def cases(llama_online_model):
    return lists_of(llama_online_model)


@pytest.fixture(scope="module")
def solved(llama_online_model, cases):
    return {name: solve_cases(llama_online_model, cs) for name, cs in cases.items()}


def check_point(model, k, w0, p, pt, want, lo=None, hi=None, tag=None):
    """One frontier point against the oracle's objective (None: no plan) and its own constraints."""
    if want is None:
        assert pt.plan is None and pt.obj_value == math.inf and pt.loaded == 0 and pt.released == 0, (tag, p, pt)
        return
    assert pt.plan is not None, (tag, p)
    assert pt.released_budget == p and pt.plan.k == k and pt.plan.obj_value == pt.obj_value
    assert bc.rel(pt.obj_value, want) <= 1e-9, (tag, p, pt.obj_value, want)
    w, n, W = pt.plan.w, pt.plan.n, int(model.L) // k
    assert sum(w) == W and all(1 <= a <= W for a in w) and all(0 <= b <= a for a, b in zip(w, n)), (tag, p, w, n)
    if lo is not None:
        assert all(a >= b for a, b in zip(w, lo)), (tag, p)
    if hi is not None:
        assert all(a <= b for a, b in zip(w, hi)), (tag, p)
    assert pt.released == cc.released(w, w0) <= p, (tag, p, w, w0)
    assert pt.loaded == sum(max(0, a - b) for a, b in zip(w, w0)) == W - sum(w0) + pt.released, (tag, p)


def check_prices(model, lists, frontiers, tag):
    """Every returned plan priced by halda_evaluate_plan on its materialised list equals its point's objective bit
    for bit (one call); the frontier is non-increasing."""
    devs, plans, objs = [], [], []
    for listed, fr in zip(lists, frontiers):
        last = math.inf
        for pt in fr:
            assert pt.obj_value <= last, (tag, pt)
            last = pt.obj_value
            if pt.plan is not None:
                devs.append(listed)
                plans.append((pt.plan.k, pt.plan.w, pt.plan.n))
                objs.append(pt.obj_value)
    if plans:
        for e, o, p in zip(pl.halda_evaluate_plans_batch(devs, model, plans, KVB), objs, plans):
            assert e.feasible and e.obj_value == o, (tag, p, e.obj_value, o)


# ------------------------------------------------------------------ 1. the case lists against the golden file
@pytest.mark.parametrize("name", ["A", "B", "W", "S", "P"])
def test_every_list_case_equals_the_oracle(llama_online_model, cases, solved, name):
    """Every recorded point within 1e-9, feasibility exactly, every point under its own constraints, every plan
    priced by halda_evaluate_plan bit for bit."""
    model, gold = llama_online_model, cc.golden()[name]
    assert len(cases[name]) == len(gold)
    for key, devs, keep, k, w0, ps in cases[name]:
        g, fr = gold[key], solved[name][key]
        assert g["w0"] == w0 and len(fr) > max(ps)  # (one launch per k: the largest budget of its lists)
        for p in ps:
            check_point(model, k, w0, p, fr[p], g["obj"][str(p)], tag=(name, key))
        for p, pt in enumerate(fr):  # the points without a recorded answer keep their own constraints
            check_point(model, k, w0, p, pt, pt.obj_value if pt.plan else None, tag=(name, key))
            assert pt.plan is None or pt.regret >= -1e-12 * max(1.0, abs(pt.obj_value)), (name, key, p)
    check_prices(model, [[c[1][j] for j in c[2]] for c in cases[name]], [solved[name][c[0]] for c in cases[name]],
                 name)


# ------------------------------------------------------------------ 2. the kernel's own outputs
def raw_call(model, parents, items, k, w0s, P, los=None, his=None, max_deficit=None):
    """One halda_solve_change_host call: (ChangeSolve, packed items)."""
    table = fleet_table(parents, model)
    packed = pack_items(table.sizes(), items)
    lens = np.diff(packed[1])
    w0 = np.concatenate([np.asarray(w, np.int32) for w in w0s])
    lo = None if los is None else ch._flat_lists((los, lens), 0)
    hi = None if his is None else ch._flat_lists((his, lens), ch.INT32_MAX)
    return ch.solve_change_table(table, model, k, packed, w0, P, bc.KV, lo, hi, max_deficit), packed


def check_raw(model, parents, items, k, w0s, P, los=None, his=None, tag=None):
    """The raw halda_change_frontier of the items gathered from their parents: (1) equal, array for array and bit
    for bit, to the call on the same lists materialised as their own table (identity items); (2) on OPTIMAL
    points obj is halda_eval_plans' device-formed objective of the returned (k, w, n) on the materialised list bit
    for bit, sum w = W, released <= p and loaded = D + released; elsewhere obj = +inf and everything is zero."""
    res, packed = raw_call(model, parents, items, k, w0s, P, los, his)
    lists = [[parents[f][j] for j in s] for f, s in items]
    mat, _ = raw_call(model, lists, [(i, list(range(len(s)))) for i, s in enumerate(lists)], k, w0s, P, los, his)
    for f in ("status", "obj", "loaded", "released", "w", "n"):
        assert np.array_equal(getattr(res, f), getattr(mat, f)), (tag, f)
    table = fleet_table(lists, model)
    karr, off, W = np.full(len(lists), k, np.int32), packed[1], int(model.L) // k
    for p in range(P + 1):
        buf = pl.evaluate_table(table, model, karr, res.w[p], res.n[p], bc.KV)
        for i in range(len(lists)):
            a, b = int(off[i]), int(off[i + 1])
            w0 = np.asarray(w0s[i])
            if res.status[i, p] == lh.STATUS_OPTIMAL:
                assert buf.status[i] == lh.STATUS_OPTIMAL and res.obj[i, p] == buf.obj[i], (tag, i, p)
                assert res.w[p, a:b].sum() == W and res.w[p, a:b].min() >= 1, (tag, i, p)
                assert res.released[i, p] == np.maximum(0, w0 - res.w[p, a:b]).sum() <= p, (tag, i, p)
                assert res.loaded[i, p] == np.maximum(0, res.w[p, a:b] - w0).sum() == W - w0.sum() + res.released[i, p]
            else:
                assert res.status[i, p] == lh.STATUS_INFEASIBLE, (tag, i, p)
                assert res.obj[i, p] == math.inf and res.loaded[i, p] == 0 and res.released[i, p] == 0, (tag, i, p)
                assert not res.w[p, a:b].any() and not res.n[p, a:b].any(), (tag, i, p)
    assert (res.obj[:, 1:] <= res.obj[:, :-1]).all(), tag  # the device-formed frontier is non-increasing
    return res


@pytest.mark.parametrize("name", ["A", "B", "S", "P"])
def test_kernel_outputs_gathered_materialised_and_priced(llama_online_model, cases, solved, name):
    """Per k one raw call of a list's cases (mixed lengths where the list has them): check_raw's identities, the
    recorded points within 1e-9, and the Python frontier carries exactly the kernel's plans."""
    model, gold = llama_online_model, cc.golden()[name]
    for k in sorted({c[3] for c in cases[name]}):
        sub = [c for c in cases[name] if c[3] == k]
        parents, at = [], {}
        for c in sub:
            if id(c[1]) not in at:
                at[id(c[1])] = len(parents)
                parents.append(c[1])
        P = max(max(c[5]) for c in sub)
        res = check_raw(model, parents, [(at[id(c[1])], c[2]) for c in sub], k, [c[4] for c in sub], P, tag=(name, k))
        assert (res.status == lh.STATUS_OPTIMAL).all()
        a = 0
        for i, c in enumerate(sub):
            for p in c[5]:
                assert bc.rel(res.obj[i, p], gold[c[0]]["obj"][str(p)]) <= 1e-9, (c[0], p)
                assert solved[name][c[0]][p].plan.w == res.w[p, a:a + len(c[2])].tolist(), (c[0], p)
            a += len(c[2])


EDGES = ["largest_deficit", "lost_head", "one_survivor", "two_lost", "joiner_no_deficit", "joiner_and_loss",
         "w_max_blocks_small_p", "crossing_box", "clipped_window", "tied_k2"]


@pytest.mark.parametrize("name", EDGES)
def test_edge_shape(llama_online_model, name):
    model = llama_online_model
    e, g = cc.edge_cases(model)[name], cc.golden()["edge"][name]["obj"]
    listed = [e["devs"][j] for j in e["idx"]]
    fr = ch.halda_change_frontiers([e["devs"]], model, [(0, e["idx"])], e["k"], [e["w0"]], e["P"], KVB,
                                   None if e["w_min"] is None else [e["w_min"]],
                                   None if e["w_max"] is None else [e["w_max"]])[0]
    assert len(fr) == e["P"] + 1
    for p, pt in enumerate(fr):
        check_point(model, e["k"], e["w0"], p, pt, g[str(p)], e["w_min"], e["w_max"], tag=name)
    check_prices(model, [listed], [fr], name)
    res = check_raw(model, [e["devs"]], [(0, e["idx"])], e["k"], [e["w0"]], e["P"],
                    None if e["w_min"] is None else [e["w_min"]], None if e["w_max"] is None else [e["w_max"]], tag=name)
    for p in range(e["P"] + 1):
        assert (res.status[0, p] == lh.STATUS_OPTIMAL) == (g[str(p)] is not None), (name, p)
    if name == "one_survivor":
        assert all(pt.plan.w == [int(model.L)] and pt.released == 0 for pt in fr)
    if name == "joiner_no_deficit":
        assert fr[0].plan is None and all(pt.plan.w[-1] >= 1 and pt.released >= 1 for pt in fr[1:])
        # the entry an operator calls gives the same frontier
        devs, w = e["devs"][:4], e["w0"][:4]
        assert ch.halda_join_frontiers(devs, [e["devs"][4]], model, (1, w, [0] * 4), e["P"], KVB)[0] == fr
    if name == "w_max_blocks_small_p":
        assert [pt.plan is None for pt in fr] == [True, True, False, False]
        assert all(a <= b for pt in fr[2:] for a, b in zip(pt.plan.w, e["w_max"]))
    if name == "two_lost":
        devs, w = cc.parent(model, 5, 1, 1)
        inc = (1, w, [0] * 5)
        assert ch.halda_failover_frontiers(devs, model, inc, e["P"], [(1, 3)], KVB)[0] == fr
        plan = ch.halda_failover_plan(devs, model, inc, (3, 1), e["P"], KVB)
        assert plan.w == fr[-1].plan.w and plan.obj_value == fr[-1].obj_value
    if name == "crossing_box":
        assert all(pt.plan is None and pt.regret == math.inf for pt in fr)


def test_mixed_lengths_in_one_call_equal_the_single_calls(llama_online_model, cases, solved):
    """Lists of 3, 4, 7 and 15 devices in one launch: each frontier equals its own call's, object for object."""
    model = llama_online_model
    pick = [next(c for c in cases[n] if len(c[1]) == M and c[3] == 2) for n, M in (("A", 4), ("A", 5), ("B", 8),
                                                                                  ("B", 16))]
    got = solve_cases(model, pick, P=3)
    for c in pick:
        one = ch.halda_change_frontiers([c[1]], model, [(0, c[2])], 2, [c[4]], 3, KVB)[0]
        assert one == got[c[0]], c[0]
        name = "A" if len(c[1]) <= 5 else "B"
        assert [pt.obj_value for pt in one[:3]] == [pt.obj_value for pt in solved[name][c[0]][:3]]  # another P


# ------------------------------------------------------------------ 3. D = 0, w0 >= 1: the budget kernel's bits
def budget_identity(model, fleets, k, w0s, P, los=None, his=None, tag=None):
    table = fleet_table(fleets, model)
    w0 = np.concatenate([np.asarray(w, np.int32) for w in w0s])
    lo = None if los is None else bg._flat(table, los, 0)
    hi = None if his is None else bg._flat(table, his, bg.INT32_MAX)
    want = bg.solve_budget_table(table, model, k, w0, P, bc.KV, lo, hi)
    items = (np.arange(table.n_fleets, dtype=np.int32), table.dev_off.astype(np.int64),
             np.concatenate([np.arange(m, dtype=np.int32) for m in table.sizes()]))
    got = ch.solve_change_table(table, model, k, items, w0, P, bc.KV, lo, hi, 0)
    for f in ("status", "obj", "w", "n"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), (tag, f)
    assert np.array_equal(got.loaded + got.released, want.moved) and np.array_equal(got.loaded, got.released), tag
    return want


def test_no_deficit_equals_the_budget_kernel_bit_for_bit(llama_online_model):
    """budget_cases' list A, one call per k (fleets of 3 and 4 devices in one launch), P = 3."""
    model, gold = llama_online_model, bu.golden()["A"]
    for k in sorted({c[1] for c in bu.LIST_A}):
        sub = [c for c in bu.LIST_A if c[1] == k]
        want = budget_identity(model, [list(bc.devices(M, s)) for M, _, s in sub], k,
                               [gold[bu.key(*c)]["w0"] for c in sub], max(bu.PS_A), tag=("A", k))
        assert (want.status == lh.STATUS_OPTIMAL).all() and (want.moved[:, -1] > 0).any()


@pytest.mark.parametrize("name", ["cap_excludes_w0", "clipped_window", "tied_k2", "one_device"])
def test_no_deficit_equals_the_budget_kernel_on_its_edge_shapes(llama_online_model, name):
    model = llama_online_model
    e = bu.edge_cases(model)[name]
    want = budget_identity(model, [e["devs"]], e["k"], [e["w0"]], e["P"], None if e["w_min"] is None else [e["w_min"]],
                           None if e["w_max"] is None else [e["w_max"]], tag=name)
    if name == "cap_excludes_w0":
        assert want.status[0].tolist() == [lh.STATUS_INFEASIBLE] * 2 + [lh.STATUS_OPTIMAL] * 2


# ------------------------------------------------------------------ 4. the far end: the free re-solve
# The lists whose free optimum at k takes more layers off the survivors than the gate admits for their width and
# deficit (cc.gate_p): {golden key: released layers of the free optimum}, by the exact oracle
# (tests/golden/change.json "free_released"). No launch can reach them; every other case is checked.
BEYOND_THE_GATE = {"S": {"4,1,0,1": 72, "4,1,0,2": 72, "5,1,0,1": 72, "5,1,0,2": 72, "5,1,0,4": 72}}


@pytest.mark.parametrize("name", ["A", "B", "S", "P"])
def test_far_end_equals_the_free_resolve(llama_online_model, cases, name):
    """Where the free optimum of the list at k releases r <= the largest admissible P, point r (and every later
    one) equals halda_solve_subfleets(..., k_candidates=[k]) within 1e-12 (DESIGN.md section 4.5's cross-path
    bound) and, r being the unique optimum's, point r - 1 is worse; no point anywhere beats the free optimum."""
    model, gold = llama_online_model, cc.golden()[name]
    beyond, reached = {}, 0
    for k in sorted({c[3] for c in cases[name]}):
        sub = [c for c in cases[name] if c[3] == k]
        parents, at = [], {}
        for c in sub:
            if id(c[1]) not in at:
                at[id(c[1])] = len(parents)
                parents.append(c[1])
        items = [(at[id(c[1])], c[2]) for c in sub]
        free = halda_solve_subfleets(parents, model, items, [k], kv_bits=KVB)
        for M in sorted({len(c[2]) for c in sub}):
            grp = [(c, it, b) for c, it, b in zip(sub, items, free) if len(c[2]) == M]
            rel = [cc.released(b.w, c[4]) for c, _, b in grp]
            Dtop = max(gold[c[0]]["D"] for c, _, _ in grp)
            P = min(cc.gate_p(ch, M, Dtop, k), max(rel))
            wide = ch.halda_change_frontiers(parents, model, [it for _, it, _ in grp], k, [c[4] for c, _, _ in grp],
                                             P, KVB)
            for (c, _, b), r, fw in zip(grp, rel, wide):
                g = gold[c[0]]
                if g["free_unique"]:
                    assert r == g["free_released"], (c[0], r)
                assert all(pt.obj_value >= b.obj_value - 1e-12 * max(1.0, abs(b.obj_value)) for pt in fw), c[0]
                if r > P:
                    beyond[c[0]] = r
                    continue
                reached += 1
                assert bc.rel(fw[r].obj_value, b.obj_value) <= 1e-12, (c[0], r, fw[r].obj_value, b.obj_value)
                assert all(pt.obj_value == fw[r].obj_value for pt in fw[r:]), c[0]
                assert abs(fw[r].regret) <= 1e-12 * max(1.0, abs(b.obj_value)), c[0]
                if r and g["free_unique"]:
                    assert fw[r - 1].obj_value > fw[r].obj_value, c[0]  # unique optimum: one layer fewer is worse
    assert beyond == BEYOND_THE_GATE.get(name, {}) and reached == len(cases[name]) - len(beyond)
    assert 3 * reached >= 2 * len(cases[name])


# ------------------------------------------------------------------ 5. rejected inputs, the C gate, the code object
def test_c_entry_rejects_what_is_outside_the_gate(llama_online_model):
    from distilp_amd.solver.fleets import HaldaChangeC, HaldaChangeFrontierC, _host_struct, model_struct
    from distilp_amd.solver.subfleets import HaldaSubfleetsC

    model = llama_online_model
    ctx = lh.get_context(0)
    lib = ctx.lib
    table = fleet_table([list(bc.devices(4, 0))], model)
    fs, keep = _host_struct(table)
    m = model_struct(model, bc.KV)
    W, P1 = int(model.L), 64
    st, obj = np.full(P1, -9, np.int32), np.zeros(P1)
    ld, rl, w, n = (np.zeros(P1 * 4, np.int32) for _ in range(4))
    fr = HaldaChangeFrontierC(3, st.ctypes.data, obj.ctypes.data, ld.ctypes.data, rl.ctypes.data, w.ctypes.data,
                              n.ctypes.data)
    parent = np.zeros(1, np.int32)

    def call(w0, max_p, max_deficit=-1, k=1, idx=(0, 1, 3), lens=(0, 0)):
        a, ix, off = np.asarray(w0, np.int32), np.asarray(idx, np.int32), np.asarray([0, len(idx)], np.int64)
        it = HaldaSubfleetsC(1, lens[0], lens[1], parent.ctypes.data, off.ctypes.data, ix.ctypes.data)
        c = HaldaChangeC(a.ctypes.data, None, None, max_p, max_deficit)
        with ctx._lock:
            return lib.halda_solve_change_host(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it), k,
                                               ctypes.byref(c), ctypes.byref(fr))

    assert call([W - 9, 1, 1], 2) == 0 and (st[:3] == lh.STATUS_OPTIMAL).all() and (ld[:3] >= 7).all()
    assert call([W - 9, 1, 1], 2, max_deficit=7) == 0 and call([W - 9, 1, 1], 2, lens=(3, 3)) == 0
    st[:] = -9
    assert call([W - 9, 1, 1], 2, max_deficit=6) == -22 and "deficit" in lh.last_error(lib)  # D above max_deficit
    assert call([W, 1, 1], 2) == -22 and "deficit" in lh.last_error(lib)  # D < 0
    assert call([W - 9, -1, 1], 2) == -22  # w0_i < 0
    assert call([W - 9, 1, 1], 64) == -22 and "max_p" in lh.last_error(lib)
    assert call([W - 9, 1, 1], 63) == 0  # D = 7 on three devices: within the gate
    st[:] = -9
    assert call([1, 1, 1, 1], 63, idx=(0, 1, 2, 3)) == -22 and "LDS" in lh.last_error(lib)  # the computed D = 76
    assert call([W - 9, 1, 1], 2, max_deficit=300) == -22 and "254" in lh.last_error(lib)
    assert call([W - 9, 1, 1], -1) == -22 and call([W - 9, 1, 1], 2, max_deficit=-2) == -22
    assert call([W - 9, 1, 1], 2, k=0) == -22
    assert call([W - 9, 1, 1], 2, idx=(0, 1, 4)) == -22 and "lists device" in lh.last_error(lib)
    assert call([W - 9, 1, 1], 2, lens=(2, 3)) == -22
    assert (st == -9).all()  # nothing was written by a rejected call
    del keep
    devs = list(bc.devices(4, 0))
    with pytest.raises(ValueError):
        ch.halda_change_frontier(devs, model, 1, [W, 1, 0, 0], 2)
    with pytest.raises(ValueError):
        ch.solve_change_table(table, model, 1, pack_items(table.sizes(), [(0, [0, 1])]), np.asarray([W - 9, 1]), 2,
                              bc.KV, max_deficit=3)


def test_change_kernel_code_object(tmp_path):
    """No spilled VGPR, no scratch, and within the VGPR budget of the two waves per SIMD its __launch_bounds__
    names (256)."""
    r = kernel_resources(tmp_path)["halda_sweep_change_kernel"]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 256, r


# ------------------------------------------------------------------ 6. a resident table
def test_launch_with_change_and_a_relaunch_with_rewritten_w0(llama_online_model):
    import torch

    dev = torch.device("cuda", 0)
    model, k, P = llama_online_model, 2, 3
    ctx = lh.get_context(0)
    devs, w = cc.parent(model, 8, 2, 11)
    items = [(0, cc.lose(devs, w, i)[0]) for i in range(8)]
    w0s = [cc.lose(devs, w, i)[2] for i in range(8)]
    table = fleet_table([devs], model)
    packed = pack_items(table.sizes(), items)
    w0 = np.concatenate([np.asarray(a, np.int32) for a in w0s])
    top = max(int(model.L) // k - sum(a) for a in w0s)
    want = ch.solve_change_table(table, model, k, packed, w0, P, bc.KV)
    dt = DeviceFleetTable(table, model, [k], bc.KV, dev)
    for bad in ((64, top), (3, 260), (-1, top)):  # the Python gate
        with pytest.raises(ValueError):
            dt.set_change(k, packed, w0, bad[0], bad[1])
    with pytest.raises(ValueError):
        dt.set_change(k, packed, w0, P, top - 1)  # a deficit above max_deficit
    dt.set_change(k, packed, w0, P, top + 4)  # a looser max_deficit changes nothing
    s = torch.cuda.Stream(dev)
    dt.launch_with_change(ctx, s.cuda_stream)
    torch.cuda.synchronize(dev)
    for f in ("status", "obj", "loaded", "released", "w", "n"):
        assert np.array_equal(dt.change_out[f].cpu().numpy(), getattr(want, f)), f
    # rewritten in place: every survivor one layer lighter where it can be (the deficit grows; within max_deficit)
    w1 = w0.copy()
    for i in range(8):
        a = int(packed[1][i])
        j = a + int(np.argmax(w0[a:int(packed[1][i + 1])]))
        w1[j] -= 1
    with torch.cuda.stream(s):
        dt.change_w0.copy_(torch.from_numpy(w1).to(dev))
    dt.launch_with_change(ctx, s.cuda_stream)
    torch.cuda.synchronize(dev)
    again = ch.solve_change_table(table, model, k, packed, w1, P, bc.KV, max_deficit=top + 4)
    for f in ("status", "obj", "loaded", "released", "w", "n"):
        assert np.array_equal(dt.change_out[f].cpu().numpy(), getattr(again, f)), f
    assert (again.loaded[:, 0] == want.loaded[:, 0] + 1).all()


# ------------------------------------------------------------------ 7. the CLI lines
def test_cli_failover_lines(llama_online_model):
    model = llama_online_model
    devs, w = cc.parent(model, 5, 2, 9)
    lines = cli.failover_lines(devs, model, (2, w, [0] * 5), 3)
    frs = ch.halda_failover_frontiers(devs, model, (2, w, [0] * 5), 3, kv_bits=KVB)
    assert len(lines) == 5
    for d, fr, line in zip(devs, frs, lines):
        pt = fr[-1]
        assert line == (f"lose {d.name}: p=3, loaded={pt.loaded}, released={pt.released}, obj={pt.obj_value:.6f}, "
                        f"regret={pt.regret:.6f}")
    assert any(fr[-1].released > 0 for fr in frs)
    lone = cli.failover_lines(devs[:2], model, (1, [int(model.L) - 1, 1], [0, 0]), 0)
    assert len(lone) == 2 and all(x.startswith("lose ") for x in lone)
