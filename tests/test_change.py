"""The change frontier without a GPU: the two oracles against each other and against tests/golden/change.json, the
argument checks (every ValueError before any GPU work), the host gate, the item packing, the exports and the CLI."""

import ctypes
import math

import numpy as np
import pytest

import distilp.solver as alias
import distilp_amd.solver as pkg
from distilp_amd.cli import solver as cli
from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import change as ch
from distilp_amd.solver.subfleets import pack_items

from . import bounds_cases as bc
from . import change_cases as cc


# ------------------------------------------------------------------ the oracles
def test_enumeration_and_highs_agree_on_the_small_lists(llama_online_model):
    """Oracle (a) against oracle (b) (cc.answer asserts 1e-9 and equal feasibility) on a sample of list A, list S
    and the pressured 5-device parent, every device lost in turn, and the answers equal the golden file's."""
    model, gold, n = llama_online_model, cc.golden(), 0
    sample = [("A", c, cc.parent(model, *c)) for c in ((4, 2, 16), (5, 4, 8), (5, 1, 0))]
    sample += [("S", c, cc.stale_parent(model, *c)) for c in ((4, 1, 1), (5, 2, 0))]
    for name, (M, k, s), (devs, w) in sample:
        for lost in range(M):
            _, listed, w0 = cc.lose(devs, w, lost)
            g = gold[name][cc.key(M, k, s, lost)]
            assert g["w0"] == w0 and g["D"] == int(model.L) // k - sum(w0)
            a = cc.answer(model, listed, k, w0, cc.PS_A, "ab", tag=(name, M, k, s, lost))
            for p in cc.PS_A:
                assert a[p] is not None and bc.rel(a[p], g["obj"][str(p)]) <= 1e-12, (name, M, k, s, lost, p)
                n += 1
    assert n == 4 * (4 + 5 + 5 + 4 + 5)


def test_golden_lists_are_complete_and_bind():
    """Every case of every list is recorded, every frontier is non-increasing, and the budget binds where it can:
    every (M, k > 1) group and every list S group has a step that strictly improves."""
    gold = cc.golden()
    want = {"A": [cc.key(M, k, s, i) for M, k, s in cc.LIST_A for i in range(M)],
            "B": [cc.key(M, k, s, i) for M, k, s in cc.LIST_B for i in range(M)],
            "S": [cc.key(M, k, s, i) for M, k, s in cc.LIST_S for i in range(M)],
            "W": [cc.key(*cc.WIDE, i) for i in range(64)],
            "P": [cc.key_p(M, sc, k, s, i) for M, sc, k, s in cc.LIST_P for i in range(M)]}
    groups = {}
    for name, keys in want.items():
        assert set(gold[name]) == set(keys), name
        for key in keys:
            f = key.split(",")
            o = [v for _, v in sorted((int(p), v) for p, v in gold[name][key]["obj"].items())]
            assert all(v is not None for v in o), key
            assert all(b <= a + 1e-9 * max(1.0, abs(a)) for a, b in zip(o, o[1:])), key
            g = groups.setdefault((name, f[0], f[-3]), [0, 0])
            g[0] += sum(b < a for a, b in zip(o, o[1:]))
            g[1] += len(o) - 1
    for (name, M, k), (better, steps) in groups.items():
        assert better >= 1 or (name != "S" and k == "1"), (name, M, k, better, steps)
    assert groups[("S", "5", "1")][0] >= 20


def test_golden_edge_shapes(llama_online_model):
    """The edge shapes' recorded answers have the shape each was built for."""
    model = llama_online_model
    edges, g = cc.edge_cases(model), cc.golden()["edge"]
    assert set(g) == set(edges)
    obj = {n: [g[n]["obj"][str(p)] for p in range(edges[n]["P"] + 1)] for n in g}
    assert obj["joiner_no_deficit"][0] is None and all(v is not None for v in obj["joiner_no_deficit"][1:])
    assert obj["w_max_blocks_small_p"][:2] == [None, None] and obj["w_max_blocks_small_p"][2] is not None
    assert all(v is None for v in obj["crossing_box"])
    assert len(set(obj["one_survivor"])) == 1 and obj["one_survivor"][0] is not None
    for name in ("clipped_window", "tied_k2"):
        assert all(b < a for a, b in zip(obj[name], obj[name][1:])), name  # the budget binds at every step
    e = edges["clipped_window"]
    W, D = int(model.L) // e["k"], int(model.L) // e["k"] - sum(e["w0"])
    assert e["w0"][0] - e["P"] < 1 and e["w0"][2] + D + e["P"] > W
    e = edges["largest_deficit"]
    assert int(model.L) - sum(e["w0"]) == max(cc.parent(model, 4, 1, 0)[1])
    e = edges["lost_head"]
    assert not any(e["devs"][j].is_head for j in e["idx"]) and any(d.is_head for d in e["devs"])
    assert len(edges["two_lost"]["idx"]) == 3 and sum(edges["joiner_no_deficit"]["w0"]) == int(model.L)


def test_deviations():
    assert sorted(cc.deviations([2, 2], 0, 1)) == [((-1, 1), 1), ((0, 0), 0), ((1, -1), 1)]
    assert sorted(d for d, _ in cc.deviations([1, 1], 2, 1)) == [(0, 2), (1, 1), (2, 0)]  # w >= 1: nothing to release
    for w0, D, p in (([3, 2, 4], 2, 2), ([0, 5, 1], 1, 3)):
        got = cc.deviations(w0, D, p)
        assert len(got) == len({d for d, _ in got})
        brute = [d for d in np.ndindex(*(2 * p + D + 1,) * 3)]
        brute = [tuple(int(v) - p for v in d) for d in brute]
        brute = [d for d in brute if sum(d) == D and sum(max(0, -v) for v in d) <= p
                 and all(a + b >= 1 for a, b in zip(w0, d))]
        assert sorted(d for d, _ in got) == sorted(brute)
        assert all(r == sum(max(0, -v) for v in d) for d, r in got)


# ------------------------------------------------------------------ the argument checks: no GPU is touched
@pytest.fixture()
def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    for name in ("get_context", "halda_evaluate_plans_batch", "fleet_table", "halda_solve_subfleets"):
        monkeypatch.setattr(ch, name, boom)


def test_entries_raise_before_any_gpu_work(llama_online_model, no_gpu):
    model = llama_online_model
    devs = list(bc.devices(4, 0))
    W = int(model.L)
    inc = (1, [W - 3, 1, 1, 1], [0, 0, 0, 0])
    with pytest.raises(ValueError, match=">= 0"):
        ch.halda_change_frontier(devs, model, 1, [W - 10, -1, 1, 1], 2)  # w0_i < 0
    with pytest.raises(ValueError, match="negative deficit"):
        ch.halda_change_frontier(devs, model, 1, [W, 1, 0, 0], 2)  # D < 0
    with pytest.raises(ValueError, match="negative deficit"):
        ch.halda_change_frontier(devs, model, 2, [W // 2, 1, 0, 0], 2)  # W is L // k
    with pytest.raises(ValueError, match="entries for a list"):
        ch.halda_change_frontier(devs, model, 1, [W - 3, 1, 1], 2)
    with pytest.raises(ValueError, match="positive integer"):
        ch.halda_change_frontier(devs, model, 0, [W - 3, 1, 1, 1], 2)
    for bad in (2.0, "4", True, None):
        with pytest.raises(ValueError, match="not an integer"):
            ch.halda_change_frontier(devs, model, 1, [W - 3, 1, 1, 0], bad)
    with pytest.raises(ValueError, match=">= 0"):
        ch.halda_change_frontier(devs, model, 1, [W - 3, 1, 1, 0], -1)
    with pytest.raises(ValueError, match="exceeds 63"):
        ch.halda_change_frontier(devs, model, 1, [W - 3, 1, 1, 0], 64)
    with pytest.raises(ValueError, match="LDS"):
        ch.halda_change_frontier(devs, model, 1, [1, 1, 1, 1], 63)  # D = 76: the planes are beyond the budget
    with pytest.raises(ValueError, match="w_min"):
        ch.halda_change_frontier(devs, model, 1, [W - 3, 1, 1, 0], 2, w_min=[1, 1, 1])
    with pytest.raises(ValueError, match="w0 lists for"):
        ch.halda_change_frontiers([devs], model, [(0, [0, 1])], 1, [], 2)
    with pytest.raises(IndexError):
        ch.halda_change_frontiers([devs], model, [(0, [0, 4])], 1, [[W - 1, 0]], 2)
    with pytest.raises(ValueError, match="empty"):
        ch.halda_change_frontiers([devs], model, [(0, [])], 1, [[]], 2)
    with pytest.raises(ValueError, match="1 .. 64 devices"):
        wide = list(bc.devices(64, 0)) + [devs[1]]
        ch.halda_change_frontier(wide, model, 1, [1] * 65, 2)
    # the failover / join entries: the incumbent is budget.check_incumbent's, `lost` names devices of the fleet
    for entry in (ch.halda_failover_frontiers, lambda *a, **k: ch.halda_join_frontiers(a[0], [devs[0]], *a[1:], **k)):
        with pytest.raises(ValueError, match="incumbent"):
            entry(devs, model, None, 2)
        with pytest.raises(ValueError, match="sums to"):
            entry(devs, model, (1, [W - 4, 1, 1, 1], [0] * 4), 2)
        with pytest.raises(ValueError, match=">= 1"):
            entry(devs, model, (1, [W - 2, 0, 1, 1], [0] * 4), 2)
        with pytest.raises(ValueError, match="w_max"):
            entry(devs, model, inc, 2, w_max=[W] * 3)
    with pytest.raises(IndexError):
        ch.halda_failover_frontiers(devs, model, inc, 2, lost=[4])
    with pytest.raises(ValueError, match="leaves no device"):
        ch.halda_failover_frontiers(devs, model, inc, 2, lost=[(0, 1, 2, 3)])
    with pytest.raises(ValueError, match="names no device"):
        ch.halda_failover_frontiers(devs, model, inc, 2, lost=[()])
    with pytest.raises(ValueError, match="deficit"):
        ch.halda_failover_frontiers(devs, model, inc, 63, lost=[0])  # 2 P + D = 126 + 77 > 254
    assert ch.halda_failover_frontiers(devs[:1], model, (1, [W], [0]), 2) == []  # nobody survives a loss


def test_check_w0_and_released():
    off = np.asarray([0, 2, 5], np.int64)
    assert ch.check_w0(off, [3, 0, 1, 1, 1], 5) == 2
    assert ch.check_w0(off, [3, 2, 1, 2, 2], 5, max_deficit=0) == 0
    with pytest.raises(ValueError, match="exceeds max_deficit"):
        ch.check_w0(off, [3, 0, 1, 1, 1], 5, max_deficit=1)
    with pytest.raises(ValueError, match="item 1"):
        ch.check_w0(off, [3, 0, 4, 1, 1], 5)
    with pytest.raises(ValueError, match="entries"):
        ch.check_w0(off, [3, 0, 4, 1], 5)
    assert [ch.check_released(b) for b in (0, 1, np.int64(16))] == [0, 1, 16]
    assert ch._lost_lists(3, None) == [[0], [1], [2]] and ch._lost_lists(1, None) == []
    assert ch._lost_lists(4, [2, (3, 1), [0]]) == [[2], [1, 3], [0]]


def test_host_gate():
    """check_gate and the slice arithmetic, tested directly: the slice grows with P, with the deficit, with the
    list and with k > 1 (the H table); the gate is the 160 KiB budget, P <= 63 and 2 P + D <= 254."""
    f = ch.change_lds_bytes
    assert f(16, 8, 0, 1) < f(16, 8, 0, 2) < f(64, 8, 0, 2) and f(16, 4, 5, 2) < f(16, 8, 5, 2) < f(16, 8, 9, 2)
    # by hand, 16 devices, P = 8, D = 5, k = 2: RS = 23, S = 9 * 14 = 126; G = H = 16 * 23 * 8 = 2944; V = 2016;
    # arg = 16 * 126 = 2016; off = 64; plan = 9 * 16 = 144; nplan = 576
    assert f(16, 8, 5, 2) == 2944 + 2944 + 2016 + 2016 + 64 + 144 + 576
    # D = 4, k = 1: RS = 21 (odd already), no H, S = 9 * 13 = 117
    assert f(16, 8, 4, 1) == 16 * 21 * 8 + 2 * 117 * 8 + 16 * 117 + 64 + 144 + 576
    ch.check_gate(64, 1, 8, 20, 2)
    ch.check_gate(63, 63, 2, 74, 1)
    with pytest.raises(ValueError, match="LDS"):
        ch.check_gate(64, 64, 40, 0, 1)
    with pytest.raises(ValueError, match="exceeds 63"):
        ch.check_gate(1, 1, 64, 0, 1)
    with pytest.raises(ValueError, match="exceeds 254"):
        ch.check_gate(1, 1, 10, 235, 1)
    ch.check_gate(1, 1, 10, 234, 1)
    with pytest.raises(ValueError, match="devices"):
        ch.check_gate(65, 3, 1, 0, 1)
    with pytest.raises(ValueError, match="devices"):
        ch.check_gate(8, 0, 1, 0, 1)
    with pytest.raises(ValueError, match="max_deficit"):
        ch.check_gate(8, 8, 1, -1, 1)


def test_c_gate_equals_python_gate_and_entries_reject_bad_arguments():
    """halda_change_lds_bytes needs no context and equals the Python arithmetic; the C entries return HALDA_E_ARG
    (-22) for a NULL argument before any HIP call."""
    if not lh.LIB_PATH.exists():
        pytest.fail(f"{lh.LIB_PATH} not built (run __graft_entry__.build())")
    lib = lh.load_library()
    for a in ((1, 0, 0, 1), (16, 8, 12, 2), (64, 8, 1, 1), (64, 2, 74, 1), (16, 63, 0, 1), (64, 63, 128, 2),
              (3, 5, 7, 4), (15, 4, 30, 2)):
        assert lib.halda_change_lds_bytes(*a) == ch.change_lds_bytes(*a), a
    assert lib.halda_change_lds_bytes(0, 1, 0, 1) == -1 and lib.halda_change_lds_bytes(4, -1, 0, 1) == -1
    assert lib.halda_change_lds_bytes(4, 1, -1, 1) == -1 and lib.halda_change_lds_bytes(4, 1, 0, 0) == -1
    assert lib.halda_solve_change_host(None, None, None, None, 1, None, None) == -22
    assert "halda_solve_change_host" in lh.last_error(lib)
    assert lib.halda_solve_change(None, None, None, None, 1, None, None, None) == -22


def test_struct_layout_matches_header():
    assert ctypes.sizeof(ch.HaldaChangeC) == 32 and ch.HaldaChangeC.max_p.offset == 24
    assert ch.HaldaChangeC.max_deficit.offset == 28
    assert ctypes.sizeof(ch.HaldaChangeFrontierC) == 56 and ch.HaldaChangeFrontierC.released.offset == 32


def test_items_are_pack_items(llama_online_model, monkeypatch):
    """The failover and join entries hand halda_change_frontiers exactly the items pack_items packs: one parent,
    the survivors (or the fleet plus one pool device) in the fleet's order, w0 in list order."""
    model = llama_online_model
    devs = list(bc.devices(4, 0))
    W = int(model.L)
    seen = {}

    def spy(fleets, model_, items, k, w0s, P, *a, **kw):
        seen.update(fleets=fleets, items=items, k=k, w0s=w0s, P=P, rest=a)
        return []

    monkeypatch.setattr(ch, "halda_change_frontiers", spy)
    inc = (2, [W // 2 - 6, 1, 2, 3], [0] * 4)
    ch.halda_failover_frontiers(devs, model, inc, 3, lost=[1, (0, 3)], w_max=[9, 8, 7, 6])
    assert len(seen["fleets"]) == 1 and seen["items"] == [(0, [0, 2, 3]), (0, [1, 2])]
    assert seen["w0s"] == [[W // 2 - 6, 2, 3], [1, 2]] and seen["k"] == 2 and seen["P"] == 3
    assert seen["rest"][2] == [[9, 7, 6], [8, 7]]
    parent, off, idx = pack_items(np.asarray([4]), seen["items"])
    assert parent.tolist() == [0, 0] and off.tolist() == [0, 3, 5] and idx.tolist() == [0, 2, 3, 1, 2]
    ch.halda_join_frontiers(devs, devs[:2], model, inc, 1)
    assert len(seen["fleets"]) == 1 and len(seen["fleets"][0]) == 6
    assert seen["items"] == [(0, [0, 1, 2, 3, 4]), (0, [0, 1, 2, 3, 5])]
    assert seen["w0s"] == [[W // 2 - 6, 1, 2, 3, 0]] * 2


# ------------------------------------------------------------------ exports, alias, CLI
def test_exports_and_alias():
    for name in ("halda_change_frontier", "halda_change_frontiers", "halda_failover_frontiers",
                 "halda_join_frontiers", "halda_failover_plan", "ChangePoint"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(ch, name)
        assert getattr(alias, name) is getattr(ch, name)
    for name in ("halda_solve_change", "halda_solve_change_host", "halda_change_lds_bytes"):
        assert name in lh.EXPORTS
    assert lh.ABI_VERSION == 3  # an additive change


def test_failover_plan_is_the_last_point_or_raises(monkeypatch):
    r = pkg.HALDAResult(w=[8], n=[0], k=2, obj_value=1.25, sets={"M1": [], "M2": [], "M3": [0]})
    none = ch.ChangePoint(0, None, math.inf, 0, 0, math.inf)
    monkeypatch.setattr(ch, "halda_failover_frontiers", lambda *a, **k: [[none, ch.ChangePoint(1, r, 1.25, 4, 1, 0.5)]])
    assert ch.halda_failover_plan([None, None], None, (2, [4, 4], [0, 0]), 1, 1) is r
    monkeypatch.setattr(ch, "halda_failover_frontiers", lambda *a, **k: [[none, none]])
    with pytest.raises(RuntimeError):
        ch.halda_failover_plan([None, None], None, (2, [4, 4], [0, 0]), 1, 1)


def test_cli_parses_failover(capsys):
    p = cli._parser()
    a = p.parse_args(["--profile", "hermes_70b", "--evaluate-solution", "s.json", "--failover", "6"])
    assert a.failover == 6 and a.move_frontier is None
    assert p.parse_args(["--profile", "hermes_70b"]).failover is None
    with pytest.raises(SystemExit):
        p.parse_args(["--profile", "hermes_70b", "--failover", "six"])
    with pytest.raises(SystemExit):
        cli.main(["--profile", "hermes_70b", "--failover", "2"])  # needs --evaluate-solution
    with pytest.raises(SystemExit):
        cli.main(["--profile", "hermes_70b", "--evaluate-solution", "s.json", "--failover", "-1"])
    capsys.readouterr()


def test_cli_failover_lines(monkeypatch):
    class Dev:
        def __init__(self, name):
            self.name = name

    r = pkg.HALDAResult(w=[8], n=[0], k=2, obj_value=1.25, sets={"M1": [], "M2": [], "M3": [0]})
    frs = [[ch.ChangePoint(0, None, math.inf, 0, 0, math.inf), ch.ChangePoint(1, None, math.inf, 0, 0, math.inf)],
           [ch.ChangePoint(0, None, math.inf, 0, 0, math.inf), ch.ChangePoint(1, r, 1.25, 4, 1, 0.5)]]
    monkeypatch.setattr(ch, "halda_failover_frontiers", lambda *a, **k: frs)
    assert cli.failover_lines([Dev("a"), Dev("b")], None, (2, [4, 4], [0, 0]), 1) == [
        "lose a: infeasible", "lose b: p=1, loaded=4, released=1, obj=1.250000, regret=0.500000"]
