"""Scale-in / scale-out without a GPU: the enumeration order and counts, the per-d deficit, the gate's arithmetic
against change.check_gate, every refusal before any GPU work, the enumeration hook against brute force on
tests/golden/scale.json and change.json, and the CLI's arguments."""

import itertools
import math

import pytest

from distilp_amd.cli import solver as cli
from distilp_amd.solver import change as ch
from distilp_amd.solver import scale as sc
from distilp_amd.solver import subsets as ss

from . import bounds_cases as bc
from . import change_cases as cc
from . import scale_cases as sx


def point(p, obj):
    """A ChangePoint of the recorded objective (the plan a marker: the hook's callers read obj_value only)."""
    if obj is None:
        return ch.ChangePoint(p, None, math.inf, 0, 0, math.inf)
    return ch.ChangePoint(p, ch.HALDAResult(w=[1], n=[0], k=1, obj_value=obj, sets={}), obj, 0, 0, 0.0)


def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("GPU work before the refusal")

    monkeypatch.setattr(sc, "get_context", boom)
    monkeypatch.setattr(sc, "fleet_table", boom)
    monkeypatch.setattr(sc, "halda_change_frontiers", boom)


# ------------------------------------------------------------------ enumeration, counts, the per-d deficit
def test_enumeration_order_and_counts():
    slots = ss.droppable(6, [1, 4])
    assert slots == [0, 2, 3, 5]
    got = [g for g, _ in ss.candidate_lists(6, slots, 2)]
    assert got == [list(c) for c in itertools.combinations(slots, 2)] == sorted(got)
    assert [sc._mask(ss.combo_devices(slots, c)) for c in ss.combo_list(4, 2)] == [sc._mask(g) for g in got]
    assert sc.scale_count(4, 6, 0, 2) == 1 + 4 + 6 and sc.scale_count(4, 6, 2, 9) == 6 + 4 + 1
    assert sc.scale_count(5, 5, 0, 9) == 2 ** 5 - 1  # M - 1 limits d: the empty fleet is no candidate
    assert sc.scale_count(3, 3, 3, 3) == 0


def test_per_d_deficit_is_the_largest_over_the_candidates():
    w0, W = [7, 0, 12, 3, 9], 40
    for keep in ([], [2], [0, 2]):
        slots = ss.droppable(5, keep)
        for d in range(len(slots) + 1):
            brute = max(W - sum(w0[i] for i in kept) for _, kept in ss.candidate_lists(5, slots, d))
            assert sc.max_deficit(w0, slots, d, W) == brute, (keep, d)
    with pytest.raises(ValueError):
        sc.max_deficit(w0, [0, 1], 3, W)


def test_launch_bytes_counts_every_array():
    P1, n, ln = 4, 10, 7
    items = 4 * n + 8 * n + 4 * n * ln                      # parent, sub_off, sub_idx
    ints = 3 * 4 * n * ln                                   # w0, w_min, w_max
    per_point = (4 + 8 + 4 + 4) * n * P1                    # status, obj, loaded, released
    planes = 2 * 4 * P1 * n * ln
    assert sc.launch_bytes(ln, P1 - 1, n) == sc.FIXED_BYTES + items + ints + per_point + planes
    assert sc.launch_bytes(64, 63, 1) < sc.CHUNK_BYTES


# ------------------------------------------------------------------ the gate against change.check_gate
def test_gate_is_the_change_gate_per_d():
    """Per d of the range the change gate on that d's longest list and largest deficit -- a large d's deficit does
    not gate a small d."""
    W, k = 250, 1
    w0 = [243, 4, 3]
    for P in (5, 6):
        tops = None
        try:
            tops = sc.check_scale_gate([3], [[0, 1, 2]], [w0], W, k, 0, 1, P)
        except ValueError:
            pass
        ok = True
        for d in (0, 1):
            try:
                ch.check_gate(3 - d, 3 - d, P, sc.max_deficit(w0, [0, 1, 2], d, W), k)
            except ValueError:
                ok = False
        assert (tops is not None) == ok == (P == 5), P
        assert sc.check_scale_gate([3], [[0, 1, 2]], [w0], W, k, 0, 0, P) == [0]
    assert sc.check_scale_gate([3], [[0, 1, 2]], [w0], W, k, 0, 1, 5) == [0, 243]
    # the LDS figure: 7 survivors with a deficit of 73 at k = 1
    w8 = [73] + [1] * 7
    Pin = min(cc.gate_p(ch, 8, 0, 1), cc.gate_p(ch, 7, 73, 1))
    assert 0 < Pin < ch.MAX_P
    sc.check_scale_gate([8], [list(range(8))], [w8], 80, 1, 0, 1, Pin)
    with pytest.raises(ValueError, match="LDS"):
        sc.check_scale_gate([8], [list(range(8))], [w8], 80, 1, 0, 1, Pin + 1)
    # mixed sizes: a fleet that does not admit d takes no part in that d's gate
    assert sc.check_scale_gate([3, 5], [[0, 1, 2], [0, 1, 2, 3, 4]], [[1, 1, 1], [2, 2, 2, 2, 2]], 10, 1, 0, 3, 2) == \
        [7, 8, 9, 6]
    # 2^20 candidates
    sc.check_scale_gate([22], [list(range(1, 22))], [[59] + [1] * 21], 80, 1, 0, 10, 0)
    with pytest.raises(ValueError, match="exceed"):
        sc.check_scale_gate([22], [list(range(22))], [[59] + [1] * 21], 80, 1, 0, 10, 0)


# ------------------------------------------------------------------ refusals before any GPU work
def test_every_refusal_comes_before_any_gpu_work(llama_online_model, monkeypatch):
    no_gpu(monkeypatch)
    model = llama_online_model
    devs, w = cc.stale_parent(model, 4, 1, 0)
    inc = (1, w, [0] * 4)
    f = sc.halda_scale_in_frontier
    for bad in (dict(max_drop=-1), dict(max_drop=1.5), dict(max_drop=64), dict(max_drop=1, min_drop=2),
                dict(max_drop=4, min_drop=4), dict(max_drop=1, max_released=-1), dict(max_drop=1, max_released=True),
                dict(max_drop=1, max_released=64), dict(max_drop=1, w_min=[1, 1]), dict(max_drop=1, w_max=[9] * 5)):
        kw = dict(max_drop=1, max_released=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            f(devs, model, inc, **kw)
    with pytest.raises(IndexError):
        f(devs, model, inc, 1, 1, keep=[4])
    with pytest.raises(IndexError):
        f([], model, inc, 1, 1)
    for bad_inc in (None, (1, w[:3], [0] * 3), (1, [80, 0, 0, 0], [0] * 4), (1, [w[0] - 1] + w[1:], [0] * 4), (0, w, w)):
        with pytest.raises(ValueError):
            f(devs, model, bad_inc, 1, 1)
    with pytest.raises(ValueError):
        f(list(bc.devices(4, 0)) * 17, model, (1, [1] * 67 + [13], [0] * 68), 1, 1)  # more than 64 devices
    with pytest.raises(ValueError):
        sc.halda_scale_in_frontier_batch([devs], model, [inc, inc], 1, 1)
    with pytest.raises(ValueError):
        sc.halda_scale_in_frontier_batch([devs], model, [inc], 1, 1, keep=[[0], [1]])
    pool = list(bc.devices(7, 1))[4:]
    for bad in (-1, 4, 1.0):
        with pytest.raises(ValueError):
            sc.halda_scale_out_frontier(devs, pool, model, inc, bad, 1)
    with pytest.raises(ValueError):
        sc.halda_scale_out_frontier(devs, list(bc.devices(61, 0)), model, inc, 1, 1)  # fleet + pool above 64
    assert sc.halda_scale_in_frontier_batch([], model, [], 1, 1) == []


# ------------------------------------------------------------------ the enumeration hook against brute force
@pytest.mark.parametrize("M,k,s", sx.PARENTS + sx.EXTRA)
def test_hook_equals_brute_force_on_the_golden_pairs(llama_online_model, M, k, s):
    """Row d = 2 through the hook fed with the recorded pair frontiers: per p the recorded strict earliest minimum
    and its pair; row d = 1 (LIST_S parents) fed with change.json: the minimum over `lost`."""
    model, gold, single = llama_online_model, sx.golden(), cc.golden()["S"]
    devs, w = cc.stale_parent(model, M, k, s)

    def solve(lists):
        out = []
        for kept in lists:
            gone = tuple(i for i in range(M) if i not in kept)
            if len(gone) == 2:
                rec = gold["pairs"][sx.pair_key(M, k, s, gone)]["obj"]
            elif len(gone) == 1 and (M, k, s) in sx.PARENTS:
                rec = single[cc.key(M, k, s, gone[0])]["obj"]
            else:
                rec = {str(p): None for p in sx.PS}
            out.append([point(p, rec[str(p)]) for p in sx.PS])
        return out

    assert sx.PS == tuple(range(sx.P + 1))
    rows = sc.halda_scale_in_frontier(devs, model, (k, w, [0] * M), 2, sx.P, min_drop=1, _solve_lists=solve)
    last = math.inf
    for p in sx.PS:
        cell = gold["cells"][f"{M},{k},{s}"][str(p)]
        pt = rows[1][p]
        if cell["obj"] is None:
            assert pt.dropped == [] and pt.kept == [] and pt.point.plan is None
            continue
        # the running minimum over p may keep an earlier list where it ties; the value is the recorded minimum
        assert pt.point.obj_value == cell["obj"] <= last and len(pt.dropped) == 2, (M, k, s, p)
        last = pt.point.obj_value
        if p == 0 or gold["cells"][f"{M},{k},{s}"][str(p - 1)]["obj"] != cell["obj"]:
            assert pt.dropped == cell["pair"], (M, k, s, p)
        assert sorted(pt.dropped + pt.kept) == list(range(M))
        if (M, k, s) in sx.PARENTS:
            _, least = sx.best([single[cc.key(M, k, s, i)]["obj"][str(p)] for i in range(M)])
            assert rows[0][p].point.obj_value == least, (M, k, s, p)
    if (M, k, s) in sx.PARENTS:
        gone, plan = sc.halda_scale_in(devs, model, (k, w, [0] * M), 1, sx.P, _solve_lists=solve)
        assert gone == rows[0][-1].dropped and plan == rows[0][-1].point.plan


def test_golden_has_a_cell_the_greedy_pair_misses():
    gold = sx.golden()
    seen = set()
    for M, k, s in sx.PARENTS + sx.EXTRA:
        for p in sx.PS:
            c = gold["cells"][f"{M},{k},{s}"][str(p)]
            if c["greedy"] is not None and c["obj"] < gold["pairs"][sx.pair_key(M, k, s, c["greedy"])]["obj"][str(p)]:
                seen.add((M, k))
    assert seen == {(M, k) for M, k, _ in sx.PARENTS} - sx.NO_GAP


def test_hook_scale_out_against_the_recorded_lists(llama_online_model):
    model, gold = llama_online_model, sx.golden()["out"]
    devs, w, pool = sx.out_case(model)
    M = len(devs)

    def solve(lists):
        return [[point(p, gold[sx.out_key([i - M for i in kept if i >= M])]["obj"][str(p)]) for p in sx.PS]
                for kept in lists]

    fr = sc.halda_scale_out_frontier(devs, pool, model, (sx.OUT[1], w, [0] * M), sx.OUT_ADD, sx.P, _solve_lists=solve)
    assert len(fr) == 3 and fr[0][0].added == [] and fr[0][0].kept == list(range(M))
    for a, row in enumerate(fr):
        keys = [key for key in gold if (0 if key == "none" else len(key.split("+"))) == a]
        for p in sx.PS:
            _, least = sx.best([gold[key]["obj"][str(p)] for key in keys])
            assert (row[p].point.plan is None) == (least is None) and (least is None or row[p].point.obj_value == least)
            assert least is None or (len(row[p].added) == a and row[p].dropped == [M + j for j in range(len(pool))
                                                                                    if j not in row[p].added])
    assert fr[1][0].point.plan is None and fr[2][1].point.plan is None  # a joiner needs a layer
    # ties go by the LEFT-OUT lists: with every objective equal the last pool device joins
    flat = sc.halda_scale_out_frontier(devs, pool, model, (sx.OUT[1], w, [0] * M), 1, 1,
                                       _solve_lists=lambda ls: [[point(p, -1.0) for p in (0, 1)] for _ in ls])
    assert flat[1][0].added == [len(pool) - 1] and flat[0][0].added == []


# ------------------------------------------------------------------ the CLI's arguments
def test_cli_scale_in_arguments():
    p = cli._parser()
    a = p.parse_args(["--profile", "x", "--evaluate-solution", "f.json", "--scale-in", "2", "--failover", "3", "--keep",
                      "0", "dev-b"])
    assert a.scale_in == 2 and a.failover == 3 and a.keep == ["0", "dev-b"]
    assert p.parse_args(["--profile", "x"]).scale_in is None
    with pytest.raises(SystemExit):
        p.parse_args(["--profile", "x", "--scale-in", "two"])


def test_cli_scale_in_lines(llama_online_model, monkeypatch):
    model = llama_online_model
    devs, w = cc.stale_parent(model, 4, 1, 0)
    cells = [[sc.ScalePoint([], list(range(4)), point(0, -3.0))],
             [sc.ScalePoint([2], [0, 1, 3], point(0, -2.5))], [sc._empty(0)]]
    monkeypatch.setattr(sc, "halda_scale_in_frontier", lambda *a, **k: cells)
    lines = cli.scale_in_lines(devs, model, (1, w, [0] * 4), 2, 0, [])
    assert lines == ["scale-in 0, 0: dropped=[], loaded=0, released=0, obj=-3.000000, regret=0.000000",
                     f"scale-in 1, 0: dropped=[{devs[2].name}], loaded=0, released=0, obj=-2.500000, regret=0.000000",
                     "scale-in 2, 0: infeasible"]
