"""The budget, change and subset kernels on deep models and full-wave fleets at k > 1 (tests/deep_cases.py) against
tests/golden/deep.json: 64- and 48-device parents at L = 160, k = 2 (W = 80: every lane of the wave holds a device
in the k > 1 threshold scan), the W = M parent, and lists on the 320- and 512-layer models whose table indices
reach 254, beside the byte planes' mark 255, around incumbents above 255 layers. The checks are test_gpu_change's
and test_gpu_budget's own helpers on another model."""

import ctypes
import math

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import budget as bg
from distilp_amd.solver import change as ch
from distilp_amd.solver import halda_solve_subfleets, halda_subset_frontier
from distilp_amd.solver.fleets import DeviceFleetTable, fleet_table
from distilp_amd.solver.subfleets import pack_items

from . import bounds_cases as bc
from . import change_cases as cc
from . import deep_cases as dc
from . import subsets_cases as sc
from . import test_gpu_budget as tgb
from . import test_gpu_change as tgc

pytestmark = pytest.mark.gpu

KVB = tgc.KVB  # kv factor 0.5, bounds_cases.KV
PW = max(dc.PS_W)
MOVING = [n for n in dc.WIDE if n not in dc.FLAT]
DEEP = list(dc.deep_cases())


@pytest.fixture(scope="module")
def gold():
    return dc.golden()


@pytest.fixture(scope="module")
def wide(llama_online_model, gold):
    """{parent: (model at L, devices, k, incumbent w, [test_gpu_change case tuples of its lists])}."""
    out = {}
    for name, (_, M, s, L, k) in dc.WIDE.items():
        devs, w = dc.wide_devices(name), gold["wide"][name]["w"]
        lists = [(ln, parent, keep, k, w0, dc.PS_W) for ln, (parent, keep, w0) in dc.wide_lists(name, devs, w).items()]
        out[name] = (dc.model_at(llama_online_model, L), devs, k, w, lists)
    return out


@pytest.fixture(scope="module")
def wide_solved(wide):
    """{parent: {list: frontier}}: one halda_change_frontiers call per parent (the joiner's parent packed beside)."""
    return {name: tgc.solve_cases(m, lists, P=PW) for name, (m, _, _, _, lists) in wide.items()}


def _call_args(lists):
    """(parents, items) of case tuples for one call: each distinct parent packed once."""
    parents, at = [], {}
    for c in lists:
        if id(c[1]) not in at:
            at[id(c[1])] = len(parents)
            parents.append(c[1])
    return parents, [(at[id(c[1])], c[2]) for c in lists]


# ------------------------------------------------------------------ 1. wide parents at k > 1: the change lists
@pytest.mark.parametrize("name", list(dc.WIDE))
def test_wide_change_lists_equal_the_oracle(wide, wide_solved, gold, name):
    """Every recorded point within 1e-9, feasibility exactly, every point under its own constraints, every plan
    priced by halda_evaluate_plans_batch bit for bit, the frontier non-increasing."""
    m, devs, k, w, lists = wide[name]
    g = gold["wide"][name]["lists"]
    assert len(lists) == len(g)
    for ln, parent, keep, _, w0, ps in lists:
        fr = wide_solved[name][ln]
        assert g[ln]["w0"] == w0 and len(fr) == PW + 1 and len(keep) >= 46
        for p in ps:
            tgc.check_point(m, k, w0, p, fr[p], g[ln]["obj"][str(p)], tag=(name, ln))
        for p, pt in enumerate(fr):
            tgc.check_point(m, k, w0, p, pt, pt.obj_value if pt.plan else None, tag=(name, ln))
            assert pt.plan is None or pt.regret >= -1e-12 * max(1.0, abs(pt.obj_value)), (name, ln, p)
        if name in dc.FLAT:  # W = M: one plan; with one device lost some survivor takes its layer, none gives one
            assert all(pt.plan.w == fr[0].plan.w and pt.released == 0 and pt.loaded == g[ln]["D"] for pt in fr)
            assert min(fr[0].plan.w) == 1 and max(fr[0].plan.w) <= 1 + g[ln]["D"]
    tgc.check_prices(m, [[c[1][j] for j in c[2]] for c in lists], [wide_solved[name][c[0]] for c in lists], name)


@pytest.mark.parametrize("name", list(dc.WIDE))
def test_wide_change_kernel_outputs_gathered_materialised_and_priced(wide, wide_solved, gold, name):
    """One raw call per parent: check_raw's identities (gathered = materialised array for array, obj the plan
    evaluation's bits), the recorded points, and the Python frontier carries the kernel's plans."""
    m, devs, k, w, lists = wide[name]
    parents, items = _call_args(lists)
    res = tgc.check_raw(m, parents, items, k, [c[4] for c in lists], PW, tag=name)
    assert (res.status == lh.STATUS_OPTIMAL).all()
    a = 0
    for i, c in enumerate(lists):
        for p in c[5]:
            assert bc.rel(res.obj[i, p], gold["wide"][name]["lists"][c[0]]["obj"][str(p)]) <= 1e-9, (name, c[0], p)
            assert wide_solved[name][c[0]][p].plan.w == res.w[p, a:a + len(c[2])].tolist(), (name, c[0], p)
        a += len(c[2])


def test_a_full_wave_a_small_and_a_single_list_in_one_call_equal_the_single_calls(wide):
    """64 listed devices (the joiner's list), 63, 3 and 1 in one k = 2 launch (the launch's Dmax and mmax are the
    wide lists' and the small list's in turn): each frontier equals its own call's, object for object."""
    m, devs, k, w, lists = wide["w64"]
    W = int(m.L) // k
    join, head = (next(c for c in lists if c[0] == n) for n in ("joiner", "head"))
    assert len(join[2]) == 64 and len(head[2]) == 63
    three, one = list(bc.devices(3, 2)), list(bc.devices(1, 3))
    parents = [join[1], head[1], three, one]
    items = [(0, join[2]), (1, head[2]), (2, [0, 1, 2]), (3, [0])]
    w0s = [join[4], head[4], [W - 50, 30, 14], [W - 3]]
    got = ch.halda_change_frontiers(parents, m, items, k, w0s, PW, KVB)
    for i, (it, w0) in enumerate(zip(items, w0s)):
        single = ch.halda_change_frontiers([parents[i]], m, [(0, it[1])], k, [w0], PW, KVB)[0]
        assert single == got[i], i
        assert all(pt.plan is not None for pt in single), i
    assert all(pt.plan.w[-1] >= 1 for pt in got[0])  # the joiner takes a layer at every point
    assert got[3][0].plan.w == [W] and got[2][PW].obj_value < got[2][0].obj_value


# ------------------------------------------------------------------ 2. wide parents: the move budget
@pytest.mark.parametrize("name", list(dc.WIDE))
def test_wide_budget_equals_the_oracle(wide, gold, name):
    m, devs, k, w, _ = wide[name]
    g = gold["wide"][name]["budget"]["obj"]
    fr = bg.halda_move_frontier(devs, m, (k, w, [0] * len(w)), 2 * PW, KVB)
    assert len(fr) == PW + 1
    for p in dc.PS_W:
        tgb.check_point(m, None, k, w, p, fr[p], g[str(p)], tag=name)
    for p, pt in enumerate(fr):
        tgb.check_point(m, None, k, w, p, pt, pt.obj_value if pt.plan else None, tag=name)
    tgb.check_frontier_prices(m, [devs], [fr], name)
    res = tgb.check_raw(m, [devs], k, [w], PW, tag=name)
    assert (res.status == lh.STATUS_OPTIMAL).all() and (np.diff(res.obj, axis=1) <= 0).all()
    assert [pt.plan.w for pt in fr] == [res.w[p].tolist() for p in range(PW + 1)]
    if name in dc.FLAT:
        assert all(pt.plan.w == w and pt.moved_layers == 0 for pt in fr)
    else:
        assert fr[PW].obj_value < fr[0].obj_value and fr[PW].moved_layers > 0


@pytest.mark.parametrize("name", MOVING + ["a512_2_p1_d0"])
def test_no_deficit_equals_the_budget_kernel_bit_for_bit(llama_online_model, wide, name):
    """D = 0 on the wide k = 2 parents and on one list of the 512-layer model."""
    if name in dc.WIDE:
        m, devs, k, w, _ = wide[name]
        want = tgc.budget_identity(m, [devs], k, [w], PW, tag=name)
    else:
        e = dc.deep_cases()[name]
        want = tgc.budget_identity(dc.model_at(llama_online_model, e["L"]), [e["devs"]], e["k"], [e["w0"]], e["P"],
                                   tag=name)
    assert (want.status == lh.STATUS_OPTIMAL).all() and (want.moved[:, -1] > 0).all()


# ------------------------------------------------------------------ 3. wide lists: the far end
# The lists whose free optimum at k takes more layers off the survivors than the gate admits for their width and
# deficit (cc.gate_p): {parent: {list: released layers of the free optimum}} (deep.json "free_released").
BEYOND_THE_GATE = {}


@pytest.mark.parametrize("name", MOVING)
def test_wide_far_end_equals_the_free_resolve(wide, gold, name):
    """Where the free optimum of a list at k releases r <= the largest admissible P, point r and every later one
    equal halda_solve_subfleets(..., k_candidates=[k]) within 1e-12 (DESIGN.md section 4.5's cross-path bound);
    no point anywhere beats the free optimum."""
    m, devs, k, w, lists = wide[name]
    g = gold["wide"][name]["lists"]
    parents, items = _call_args(lists)
    free = halda_solve_subfleets(parents, m, items, [k], kv_bits=KVB)
    beyond, reached = {}, 0
    for M in sorted({len(c[2]) for c in lists}):
        grp = [(c, it, b) for c, it, b in zip(lists, items, free) if len(c[2]) == M]
        rel = [cc.released(b.w, c[4]) for c, _, b in grp]
        P = min(cc.gate_p(ch, M, max(g[c[0]]["D"] for c, _, _ in grp), k), max(rel))
        far = ch.halda_change_frontiers(parents, m, [it for _, it, _ in grp], k, [c[4] for c, _, _ in grp], P, KVB)
        for (c, _, b), r, fw in zip(grp, rel, far):
            if g[c[0]]["free_unique"]:
                assert r == g[c[0]]["free_released"], (name, c[0], r)
            assert all(pt.obj_value >= b.obj_value - 1e-12 * max(1.0, abs(b.obj_value)) for pt in fw), (name, c[0])
            if r > P:
                beyond[c[0]] = r
                continue
            reached += 1
            assert bc.rel(fw[r].obj_value, b.obj_value) <= 1e-12, (name, c[0], r, fw[r].obj_value, b.obj_value)
            assert all(pt.obj_value == fw[r].obj_value for pt in fw[r:]), (name, c[0])
            assert abs(fw[r].regret) <= 1e-12 * max(1.0, abs(b.obj_value)), (name, c[0])
            if r and g[c[0]]["free_unique"]:
                assert fw[r - 1].obj_value > fw[r].obj_value, (name, c[0])
    assert beyond == BEYOND_THE_GATE.get(name, {}) and reached == len(lists) - len(beyond)
    assert 3 * reached >= 2 * len(lists)


# ------------------------------------------------------------------ 4. deep models: the byte edge
def _deep_call(model, e, P=None):
    m = dc.model_at(model, e["L"])
    P = e["P"] if P is None else P
    return m, ch.halda_change_frontiers([e["devs"]], m, [(0, e["idx"])], e["k"], [e["w0"]], P, KVB)[0]


@pytest.mark.parametrize("name", DEEP)
def test_deep_list_equals_the_oracle(llama_online_model, gold, name):
    """A list whose table indices reach 2 P + D (254 at the edge): the recorded points within 1e-9, every point
    under its own constraints and priced bit for bit, the raw outputs gathered = materialised."""
    e, g = dc.deep_cases()[name], gold["deep"][name]
    m, fr = _deep_call(llama_online_model, e)
    assert g["w0"] == e["w0"] and len(fr) == e["P"] + 1
    for p in e["ps"]:
        tgc.check_point(m, e["k"], e["w0"], p, fr[p], g["obj"][str(p)], tag=name)
    for p, pt in enumerate(fr):
        tgc.check_point(m, e["k"], e["w0"], p, pt, pt.obj_value if pt.plan else None, tag=name)
        assert pt.plan is None or pt.loaded == e["D"] + pt.released, (name, p)
    tgc.check_prices(m, [[e["devs"][j] for j in e["idx"]]], [fr], name)
    res = tgc.check_raw(m, [e["devs"]], [(0, e["idx"])], e["k"], [e["w0"]], e["P"], tag=name)
    for p in e["ps"]:
        assert (res.status[0, p] == lh.STATUS_OPTIMAL) == (g["obj"][str(p)] is not None), (name, p)
    if len(e["idx"]) == 1:  # one device takes every layer: table index D = 254, above 255 layers at L = 512
        assert all(pt.plan.w == [e["L"] // e["k"]] and pt.loaded == e["D"] for pt in fr)


@pytest.mark.parametrize("pair", list(dc.PAIRS))
def test_the_largest_deficit_beside_no_deficit_in_one_call(llama_online_model, gold, pair):
    """Two items of one launch, D = 252 and D = 0: the second item's own LQ is not the slice's. Each equals its
    single call object for object and its recorded points."""
    cases = [dc.deep_cases()[n] for n in dc.PAIRS[pair]]
    m = dc.model_at(llama_online_model, cases[0]["L"])
    k, P = cases[0]["k"], cases[0]["P"]
    got = ch.halda_change_frontiers([e["devs"] for e in cases], m, [(i, e["idx"]) for i, e in enumerate(cases)], k,
                                    [e["w0"] for e in cases], P, KVB)
    for n, e, fr in zip(dc.PAIRS[pair], cases, got):
        assert fr == _deep_call(llama_online_model, e)[1], n
        for p in e["ps"]:
            tgc.check_point(m, k, e["w0"], p, fr[p], gold["deep"][n]["obj"][str(p)], tag=(pair, n))
    tgc.check_raw(m, [e["devs"] for e in cases], [(i, e["idx"]) for i, e in enumerate(cases)], k,
                  [e["w0"] for e in cases], P, tag=pair)


@pytest.mark.parametrize("name", list(dc.deep_budget_cases()))
def test_deep_budget_equals_the_oracle(llama_online_model, gold, name):
    """The budget kernel at its own top (P = 63: table index 126) around incumbents above 255 layers."""
    e, g = dc.deep_budget_cases()[name], gold["deep_budget"][name]["obj"]
    m, k, w0, P = dc.model_at(llama_online_model, e["L"]), e["k"], e["w0"], e["P"]
    fr = bg.halda_move_frontier(e["devs"], m, (k, w0, [0] * len(w0)), 2 * P, KVB)
    assert len(fr) == P + 1 and sorted(int(p) for p in g) == sorted(set(e["ps_a"]) | {e["top"]})
    for p in g:
        tgb.check_point(m, None, k, w0, int(p), fr[int(p)], g[p], tag=name)
    for p, pt in enumerate(fr):
        tgb.check_point(m, None, k, w0, p, pt, pt.obj_value if pt.plan else None, tag=name)
    tgb.check_frontier_prices(m, [e["devs"]], [fr], name)
    res = tgb.check_raw(m, [e["devs"]], k, [w0], P, tag=name)
    assert (res.status == lh.STATUS_OPTIMAL).all() and (np.diff(res.obj, axis=1) <= 0).all()


# ------------------------------------------------------------------ 5. one past the edge
def _c_entry(model, e, out_fill=-9):
    """halda_solve_change_host on a case as the C caller makes it (no max_deficit given): (rc, message, status)."""
    from distilp_amd.solver.fleets import HaldaChangeC, HaldaChangeFrontierC, _host_struct, model_struct
    from distilp_amd.solver.subfleets import HaldaSubfleetsC

    m = dc.model_at(model, e["L"])
    ctx = lh.get_context(0)
    lib = ctx.lib
    table = fleet_table([e["devs"]], m)
    fs, keep = _host_struct(table)
    ms = model_struct(m, bc.KV)
    P1, n = e["P"] + 1, len(e["idx"])
    st, obj = np.full(P1, out_fill, np.int32), np.full(P1, float(out_fill))
    ld, rl = np.full(P1, out_fill, np.int32), np.full(P1, out_fill, np.int32)
    w, nn = np.full(P1 * n, out_fill, np.int32), np.full(P1 * n, out_fill, np.int32)
    outs = (st, obj, ld, rl, w, nn)
    fr = HaldaChangeFrontierC(n, *(a.ctypes.data for a in outs))
    parent, off = np.zeros(1, np.int32), np.asarray([0, n], np.int64)
    ix, w0 = np.asarray(e["idx"], np.int32), np.asarray(e["w0"], np.int32)
    it = HaldaSubfleetsC(1, n, n, parent.ctypes.data, off.ctypes.data, ix.ctypes.data)
    c = HaldaChangeC(w0.ctypes.data, None, None, e["P"], -1)
    with ctx._lock:
        rc = lib.halda_solve_change_host(ctx.ctx, ctypes.byref(ms), ctypes.byref(fs), ctypes.byref(it), e["k"],
                                         ctypes.byref(c), ctypes.byref(fr))
    del keep
    return rc, lh.last_error(lib) if rc else "", outs


@pytest.mark.parametrize("name", list(dc.rejected_cases()))
def test_one_past_the_edge_is_rejected(llama_online_model, name):
    """2 P + D = 255 through a real deficit (and 64 devices at k = 2 with D = 254): ValueError from the Python
    entries, -22 with the documented word from the C entry, and no output written."""
    e = dc.rejected_cases()[name]
    m = dc.model_at(llama_online_model, e["L"])
    with pytest.raises(ValueError, match=e["error"]):
        ch.halda_change_frontiers([e["devs"]], m, [(0, e["idx"])], e["k"], [e["w0"]], e["P"], KVB)
    table = fleet_table([e["devs"]], m)
    packed = pack_items(table.sizes(), [(0, e["idx"])])
    with pytest.raises(ValueError, match=e["error"]):
        ch.solve_change_table(table, m, e["k"], packed, np.asarray(e["w0"], np.int32), e["P"], bc.KV)
    rc, msg, outs = _c_entry(llama_online_model, e)
    assert rc == -22 and e["error"] in msg, (name, rc, msg)
    assert all((a == -9).all() for a in outs), name


def test_the_c_entry_admits_the_edge_itself(llama_online_model, gold):
    """The same call shape one layer earlier (2 P + D = 254) returns 0 and the recorded point."""
    for name in ("a512_1_p0_d254", "a320_2_p1_d252"):
        e = dc.deep_cases()[name]
        rc, msg, outs = _c_entry(llama_online_model, e)
        assert rc == 0, (name, msg)
        assert (outs[0] == lh.STATUS_OPTIMAL).all() and (outs[2] >= e["D"]).all(), name
        for p in e["ps"]:
            assert bc.rel(outs[1][p], gold["deep"][name]["obj"][str(p)]) <= 1e-9, (name, p)


# ------------------------------------------------------------------ 6. resident tables
def _resident_change(m, parents, items, k, w0s, P):
    import torch

    dev = torch.device("cuda", 0)
    table = fleet_table(parents, m)
    packed = pack_items(table.sizes(), items)
    w0 = np.concatenate([np.asarray(a, np.int32) for a in w0s])
    top = max(int(m.L) // k - sum(a) for a in w0s)
    want = ch.solve_change_table(table, m, k, packed, w0, P, bc.KV)
    dt = DeviceFleetTable(table, m, [k], bc.KV, dev)
    dt.set_change(k, packed, w0, P, top)
    s = torch.cuda.Stream(dev)
    dt.launch_with_change(lh.get_context(0), s.cuda_stream)
    torch.cuda.synchronize(dev)
    for f in ("status", "obj", "loaded", "released", "w", "n"):
        assert np.array_equal(dt.change_out[f].cpu().numpy(), getattr(want, f)), f
    assert (want.status == lh.STATUS_OPTIMAL).all()
    return dt, packed, w0, top


def test_launch_with_change_on_a_wide_parent_and_at_the_byte_edge(llama_online_model, wide):
    m, devs, k, w, lists = wide["w64"]
    own = [c for c in lists if c[1] is devs]  # the lists of the one parent
    _resident_change(m, [devs], [(0, c[2]) for c in own], k, [c[4] for c in own], PW)
    cases = [dc.deep_cases()[n] for n in dc.PAIRS["pair_p1"]]
    m = dc.model_at(llama_online_model, cases[0]["L"])
    dt, packed, w0, top = _resident_change(m, [e["devs"] for e in cases], [(i, e["idx"]) for i, e in enumerate(cases)],
                                           cases[0]["k"], [e["w0"] for e in cases], cases[0]["P"])
    assert top == 252
    with pytest.raises(ValueError, match="254"):
        dt.set_change(cases[0]["k"], packed, w0, cases[0]["P"], top + 1)  # 2 P + max_deficit = 255


def _resident_budget(m, devs, k, w0, P):
    import torch

    dev = torch.device("cuda", 0)
    table = fleet_table([devs], m)
    a = np.asarray(w0, np.int32)
    want = bg.solve_budget_table(table, m, k, a, P, bc.KV)
    dt = DeviceFleetTable(table, m, [k], bc.KV, dev)
    dt.set_budget(k, a, P)
    s = torch.cuda.Stream(dev)
    dt.launch_with_budget(lh.get_context(0), s.cuda_stream)
    torch.cuda.synchronize(dev)
    for f in ("status", "obj", "moved", "w", "n"):
        assert np.array_equal(dt.budget_out[f].cpu().numpy(), getattr(want, f)), f
    assert (want.status == lh.STATUS_OPTIMAL).all()


def test_launch_with_budget_on_a_wide_parent_and_at_the_byte_edge(llama_online_model, wide):
    m, devs, k, w, _ = wide["w64"]
    _resident_budget(m, devs, k, w, PW)
    e = dc.deep_budget_cases()["m512_3_p63"]
    _resident_budget(dc.model_at(llama_online_model, e["L"]), e["devs"], e["k"], e["w0"], e["P"])


# ------------------------------------------------------------------ 7. exact device selection
@pytest.mark.parametrize("case", dc.SUBSETS, ids=dc.subset_id)
def test_subsets_on_both_paths_against_the_brute_force(gold, case):
    """The raw frontier of the automatic path and of the forced expansion equals the arg-min over every candidate's
    halda_solve_subfleets value bit for bit (check_frontier) and the recorded brute force over the exact oracle
    within 1e-9; every point's `result` of the Python entry is halda_solve_subfleets of its kept list bit for bit.
    Both paths take the expansion route: the fused route's gate (L - M + 1 <= 64) admits neither fleet."""
    from . import test_gpu_subsets as tgs

    key, D, keep = case
    devs, model, kv, ks = sc.fleet_of(key)
    M, L = len(devs), int(model.L)
    ks = [d for d in range(1, L) if L % d == 0] if ks is None else list(ks)
    # the fused route needs the register sweep (L - M + 1 <= 64 DP lanes), which no model this deep has: the
    # automatic path and the forced one both expand here, and check_frontier holds each to every candidate
    st, obj, dm, bk = tgs.check_frontier([devs], model, D, [keep], ks=ks, route0="expand")
    bf = gold["subsets"][dc.subset_id(case)]
    assert len(bf) == D + 1
    for d, (best, gone, runner) in enumerate(bf):
        assert st[0, d] == lh.STATUS_OPTIMAL and best is not None, (case, d)
        assert abs(obj[0, d] - best) <= sc.REL_OBJ * max(1.0, abs(best)), (case, d, obj[0, d], best)
        if not sc.near_tie(best, math.inf if runner is None else runner):
            assert int(dm[0, d]) == tgs.mask_of(gone), (case, d, int(dm[0, d]), gone)
    pts = halda_subset_frontier(devs, model, D, keep, k_candidates=ks, kv_bits=kv)
    same = halda_solve_subfleets([devs], model, [(0, p.kept) for p in pts], k_candidates=ks, kv_bits=kv)
    assert len(pts) == D + 1
    for d, (p, r) in enumerate(zip(pts, same)):
        assert abs(p.obj_value - bf[d][0]) <= sc.REL_OBJ * max(1.0, abs(bf[d][0])), (case, d)
        assert (p.result.k, p.result.w, p.result.n, p.result.sets) == (r.k, r.w, r.n, r.sets), (case, d)
        assert np.float64(p.result.obj_value).tobytes() == np.float64(r.obj_value).tobytes(), (case, d)
