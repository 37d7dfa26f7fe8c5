"""The total move budget without a GPU: the two oracles against each other and against tests/golden/budget.json,
the argument checks (every ValueError before any GPU work), the host gate, the exports and the CLI flag."""

import ctypes
import math

import numpy as np
import pytest

import distilp.solver as alias
import distilp_amd.solver as pkg
from distilp_amd.cli import solver as cli
from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import budget as bg

from . import bounds_cases as bc
from . import budget_cases as bu


# ------------------------------------------------------------------ the oracles
def test_enumeration_and_highs_agree_on_list_a(llama_online_model):
    """Oracle (a) against oracle (b) on M in {3, 4}: 120 points within 1e-9 relative, none skipped; the golden
    file holds (a)'s answers."""
    model, gold, n = llama_online_model, bu.golden()["A"], 0
    for M, k, s in bu.LIST_A:
        devs, w0 = bu.list_case(model, M, k, s)
        prob = bu.problem(model, devs, k)
        a = bu.enumerate_frontier(prob, w0, bu.PS_A)
        g = gold[bu.key(M, k, s)]
        assert g["w0"] == w0
        for p in bu.PS_A:
            b, w = bu.highs_budget(prob, w0, p)
            assert a[p] is not None and b is not None, (M, k, s, p)
            assert bc.rel(a[p], b) <= 1e-9, (M, k, s, p, a[p], b)
            assert bc.rel(a[p], g["obj"][str(p)]) <= 1e-12, (M, k, s, p)
            n += 1
    assert n == 120


def test_highs_and_pinned_exact_agree_on_list_b(llama_online_model):
    """Oracle (b) against the exact solver pinned on (b)'s w, M in {8, 16}: 150 points within 1e-9, none
    skipped; the budget binds (110 of the 120 steps between consecutive budgets strictly improve)."""
    model, gold, n, steps, better = llama_online_model, bu.golden()["B"], 0, 0, 0
    for M, k, s in bu.LIST_B:
        devs, w0 = bu.list_case(model, M, k, s)
        prob = bu.problem(model, devs, k)
        pin = bu.Pinned(prob)
        g = gold[bu.key(M, k, s)]
        assert g["w0"] == w0
        objs = []
        for p in bu.PS_B:
            b, w = bu.highs_budget(prob, w0, p)
            assert b is not None, (M, k, s, p)
            e = pin(w)
            assert e is not None and bc.rel(b, e) <= 1e-9, (M, k, s, p, b, e)
            assert bc.rel(e, g["obj"][str(p)]) <= 1e-12, (M, k, s, p)
            objs.append(e)
            n += 1
        steps += len(objs) - 1
        better += sum(q < p for p, q in zip(objs, objs[1:]))
        assert all(q <= p + 1e-9 * max(1.0, abs(p)) for p, q in zip(objs, objs[1:])), (M, k, s)
    assert n == 150 and steps == 120 and better == 110


def test_list_p_oracles_agree_and_the_budget_binds_under_pressure(llama_online_model):
    """List P (memory-pressured fleets): a sample recomputed -- oracle (a) against (b) on a 5-device case, (b)
    against the pinned exact solver on a 16-device case of each scale and on the 64-device fleet, each within 1e-9
    (list_p_answer asserts it) and equal to the golden -- and, over the whole recorded list, at least 80 % of the
    steps between consecutive budgets strictly improve (recorded: 86 of 89), so the frontier tests something."""
    model, gold = llama_online_model, bu.golden()["P"]
    assert set(gold) == {bu.key_p(*c) for c in bu.LIST_P} and len(bu.LIST_P) == 25
    from . import pressure_cases as pc

    for c in ((5, pc.S16, 2, 1), (5, pc.S16, 4, 0), (16, pc.S16, 2, 0), (16, pc.S64, 1, 2), (64, pc.S64, 1, 0)):
        w0, objs, fp, uniq = bu.list_p_answer(model, *c)
        g = gold[bu.key_p(*c)]
        assert g["w0"] == w0 and g["free_p"] == fp and g["free_unique"] == uniq, c
        for p in bu.ps_of_p(c[0]):
            assert bc.rel(objs[p], g["obj"][str(p)]) <= 1e-12, (c, p)
    steps = better = 0
    for c in bu.LIST_P:
        o = [gold[bu.key_p(*c)]["obj"][str(p)] for p in bu.ps_of_p(c[0])]
        assert all(v is not None for v in o), c
        assert all(b <= a + 1e-9 * max(1.0, abs(a)) for a, b in zip(o, o[1:])), c
        steps += len(o) - 1
        better += sum(b < a for a, b in zip(o, o[1:]))
    print(f"list P: {better} of {steps} steps strictly improve")
    assert steps == 89 and better >= 0.8 * steps
    # the pressured incumbents and optima do use slacks: the tables' H[i][e] are shaped by them
    used = 0
    for M, sc, k, s in bu.LIST_P:
        st, x, _, _ = pc.exact((M, sc, s, "4bit"), k)
        used += st == 0 and bool((x[2 * M:6 * M] > 0.5).any())
    assert used >= 0.9 * len(bu.LIST_P)


def test_golden_edge_shapes(llama_online_model):
    """The edge shapes' recorded answers have the shape each was built for."""
    g = bu.golden()["edge"]
    assert set(g) == set(bu.edge_cases(llama_online_model))
    cap = g["cap_excludes_w0"]["obj"]
    assert cap["0"] is None and cap["1"] is None and cap["2"] is not None and cap["3"] is not None
    assert all(v is None for v in g["crossing_box"]["obj"].values())
    one = list(g["one_device"]["obj"].values())
    assert one[0] is not None and one == [one[0]] * 3
    for name in ("clipped_window", "tied_k2", "pressured"):
        o = [g[name]["obj"][str(p)] for p in range(4)]
        assert all(b < a for a, b in zip(o, o[1:])), name  # the budget binds at every step
    cap = g["pressured_cap_excludes_w0"]["obj"]
    assert cap["0"] is None and cap["1"] is None and cap["3"] < cap["2"]
    lo = g["pressured_w_min"]["obj"]
    assert lo["0"] is None and lo["3"] < lo["2"] < lo["1"]


def test_deviations():
    assert sorted(bu.deviations(2, 1)) == [(-1, 1), (0, 0), (1, -1)]
    assert all(sum(d) == 0 and sum(v for v in d if v > 0) <= 2 for d in bu.deviations(3, 2))
    assert len(bu.deviations(3, 1)) == 7


# ------------------------------------------------------------------ the argument checks: no GPU is touched
@pytest.fixture()
def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(bg, "get_context", boom)
    monkeypatch.setattr(bg, "halda_evaluate_plans_batch", boom)
    monkeypatch.setattr(bg, "fleet_table", boom)


def test_entries_raise_before_any_gpu_work(llama_online_model, no_gpu):
    model = llama_online_model
    devs = list(bc.devices(4, 0))
    W = int(model.L)
    good = (1, [W - 3, 1, 1, 1], [0, 0, 0, 0])
    for entry in (bg.halda_move_frontier, bg.halda_solve_budget):
        with pytest.raises(ValueError, match="incumbent"):
            entry(devs, model, None, 4)
        with pytest.raises(ValueError, match="entries for a fleet"):
            entry(devs, model, (1, [W - 2, 1, 1], [0, 0, 0]), 4)  # a wrong length
        with pytest.raises(ValueError, match="sums to"):
            entry(devs, model, (1, [W - 4, 1, 1, 1], [0] * 4), 4)  # sum w0 != W
        with pytest.raises(ValueError, match="sums to"):
            entry(devs, model, (2, [W - 3, 1, 1, 1], [0] * 4), 4)  # W is L // k
        with pytest.raises(ValueError, match=">= 1"):
            entry(devs, model, (1, [W - 2, 0, 1, 1], [0] * 4), 4)  # w0_i < 1
        with pytest.raises(ValueError, match=">= 0"):
            entry(devs, model, good, -2)
        for bad in (2.0, "4", True, None):
            with pytest.raises(ValueError, match="not an integer"):
                entry(devs, model, good, bad)
        with pytest.raises(ValueError, match="exceeds 63"):
            entry(devs, model, good, 128)  # P = 64
        with pytest.raises(ValueError, match="LDS"):
            entry(devs, model, good, 126)  # P = 63 on 4 devices: the planes alone are beyond the budget
        with pytest.raises(ValueError, match="w_min"):
            entry(devs, model, good, 4, w_min=[1, 1, 1])
    with pytest.raises(ValueError, match="incumbents for"):
        bg.halda_move_frontier_batch([devs], model, [], 4)
    with pytest.raises(ValueError, match="1 .. 64 devices"):
        wide = list(bc.devices(64, 0)) + [devs[1]]
        bg.halda_move_frontier(wide, model, (1, [W - 64] + [1] * 64, [0] * 65), 2)


def test_host_gate():
    """check_gate and the slice arithmetic, tested directly: the slice grows with P, with the fleet and with
    k > 1 (the H table), and the gate is the 160 KiB budget."""
    assert bg.budget_lds_bytes(16, 8, 1) < bg.budget_lds_bytes(16, 8, 2) < bg.budget_lds_bytes(64, 8, 2)
    assert bg.budget_lds_bytes(16, 4, 2) < bg.budget_lds_bytes(16, 8, 2)
    # by hand, 16 devices, P = 8, k = 2: RS = 17, S = 153; G = H = 16 * 17 * 8 = 2176; V = 2 * 153 * 8 = 2448;
    # arg = 16 * 153 = 2448; off = 64; plan = 9 * 16 = 144; nplan = 576
    assert bg.budget_lds_bytes(16, 8, 2) == 2176 + 2176 + 2448 + 2448 + 64 + 144 + 576
    bg.check_gate(64, 1, 8, 2)
    bg.check_gate(16, 16, 40, 2)
    assert bg.budget_lds_bytes(16, 40, 2) <= bg.LDS_BUDGET < bg.budget_lds_bytes(16, 48, 2)
    with pytest.raises(ValueError, match="LDS"):
        bg.check_gate(16, 16, 48, 2)
    with pytest.raises(ValueError, match="LDS"):
        bg.check_gate(64, 64, 40, 1)
    with pytest.raises(ValueError, match="exceeds 63"):
        bg.check_gate(1, 1, 64, 1)
    with pytest.raises(ValueError, match="devices"):
        bg.check_gate(65, 3, 1, 1)
    with pytest.raises(ValueError, match="devices"):
        bg.check_gate(8, 0, 1, 1)


def test_c_gate_equals_python_gate_and_entries_reject_bad_arguments():
    """halda_budget_lds_bytes needs no context and equals the Python arithmetic; the C entries return
    HALDA_E_ARG (-22) for a NULL argument before any HIP call."""
    if not lh.LIB_PATH.exists():
        pytest.fail(f"{lh.LIB_PATH} not built (run __graft_entry__.build())")
    lib = lh.load_library()
    for M, P, k in ((1, 0, 1), (16, 8, 2), (64, 8, 1), (64, 2, 1), (16, 63, 1), (64, 63, 2), (3, 5, 4)):
        assert lib.halda_budget_lds_bytes(M, P, k) == bg.budget_lds_bytes(M, P, k), (M, P, k)
    assert lib.halda_budget_lds_bytes(0, 1, 1) == -1 and lib.halda_budget_lds_bytes(4, -1, 1) == -1
    assert lib.halda_solve_fleets_budget_host(None, None, None, 1, None, None) == -22
    assert "halda_solve_fleets_budget_host" in lh.last_error(lib)
    assert lib.halda_solve_fleets_budget(None, None, None, 1, None, None, None) == -22


def test_struct_layout_matches_header():
    assert ctypes.sizeof(bg.HaldaBudgetC) == 32 and bg.HaldaBudgetC.max_p.offset == 24
    assert ctypes.sizeof(bg.HaldaFrontierC) == 48 and bg.HaldaFrontierC.status.offset == 8


def test_check_budget_and_incumbent():
    assert [bg.check_budget(b) for b in (0, 1, 2, 7, np.int64(16))] == [0, 0, 1, 3, 8]
    assert bg.check_incumbent((np.int32(2), (3, 1), [0, 0]), 2, 8) == (2, [3, 1], [0, 0])
    r = pkg.HALDAResult(w=[3, 1], n=[1, 0], k=2, obj_value=1.0, sets={"M1": [], "M2": [], "M3": [0, 1]})
    assert bg.check_incumbent(r, 2, 8) == (2, [3, 1], [1, 0])
    with pytest.raises(ValueError):
        bg.check_incumbent((0, [3, 1], [0, 0]), 2, 8)


# ------------------------------------------------------------------ exports, alias, CLI
def test_exports_and_alias():
    for name in ("halda_move_frontier", "halda_move_frontier_batch", "halda_solve_budget", "FrontierPoint"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(bg, name)
        assert getattr(alias, name) is getattr(bg, name)
    for name in ("halda_solve_fleets_budget", "halda_solve_fleets_budget_host", "halda_budget_lds_bytes"):
        assert name in lh.EXPORTS
    assert lh.ABI_VERSION == 3  # an additive change


def test_cli_parses_move_frontier(capsys):
    p = cli._parser()
    a = p.parse_args(["--profile", "hermes_70b", "--evaluate-solution", "s.json", "--move-frontier", "6"])
    assert a.move_frontier == 6 and a.max_move is None
    assert p.parse_args(["--profile", "hermes_70b"]).move_frontier is None
    with pytest.raises(SystemExit):
        p.parse_args(["--profile", "hermes_70b", "--move-frontier", "six"])
    with pytest.raises(SystemExit):
        cli.main(["--profile", "hermes_70b", "--move-frontier", "2"])  # needs --evaluate-solution
    with pytest.raises(SystemExit):
        cli.main(["--profile", "hermes_70b", "--evaluate-solution", "s.json", "--move-frontier", "-1"])
    capsys.readouterr()


def test_cli_frontier_lines(monkeypatch):
    r = pkg.HALDAResult(w=[5, 3], n=[0, 0], k=2, obj_value=1.25, sets={"M1": [], "M2": [], "M3": [0, 1]})
    pts = [bg.FrontierPoint(0, None, math.inf, 0, -math.inf), bg.FrontierPoint(2, r, 1.25, 2, 0.5)]
    monkeypatch.setattr(bg, "halda_move_frontier", lambda *a, **k: pts)
    assert cli.frontier_lines([None, None], None, (2, [4, 4], [0, 0]), 2) == [
        "frontier 0: infeasible", "frontier 1: moved_layers=2, obj=1.250000, regret=0.500000"]
