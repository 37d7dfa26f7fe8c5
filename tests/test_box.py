"""Layer bounds on n, on the CPU: the argument checks of check_bounds / move_box, the array layout of mixed 2- and
4-tuples, the exact oracle against HiGHS on the shared cases, the pin cases against evaluate_plan_np, and the CLI's
new flags. No GPU."""

import numpy as np
import pytest

from distilp_amd.cli import solver as cli
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import fleet_table
from oracle import milp_oracle as mo

from . import bounds_cases as bc
from . import box_cases as xc

IMAX = xc.IMAX


# ------------------------------------------------------------------ argument checks
def test_check_bounds_with_n_lists():
    assert bd.check_bounds([1, 2], None, 2) == ([1, 2], None)  # without the n arguments: the pair, as before
    assert bd.check_bounds([1, 2], None, 2, None, None) == ([1, 2], None, None, None)
    assert bd.check_bounds(None, None, 2, [-1, 3], [2, 2]) == (None, None, [-1, 3], [2, 2])  # no error: no bound, crossing
    assert bd.check_bounds(None, [4, 4], 2, n_max=[0, IMAX]) == (None, [4, 4], None, [0, IMAX])
    for kw in ({"n_min": [0]}, {"n_max": [0, 0, 0]}, {"n_min": 3}):
        with pytest.raises(ValueError, match="n_m"):
            bd.check_bounds(None, None, 2, **kw)
    for bad in ([0.5, 1], [True, 1], ["1", 1]):
        with pytest.raises(ValueError, match="not an integer"):
            bd.check_bounds(None, None, 2, n_max=bad)
    with pytest.raises(ValueError, match="w_min"):
        bd.check_bounds([0, 1], None, 2, [0, 0], None)


def test_move_box():
    assert bd.move_box([3, 1], [2, 0], 1) == ([2, 1], [4, 2], None, None)
    assert bd.move_box([3, 1], [2, 0], 1, 1) == ([2, 1], [4, 2], [1, 0], [3, 1])
    assert bd.move_box([3, 1], [2, 0], [0, 2], [0, 2]) == ([3, 1], [3, 3], [2, 0], [2, 2])
    assert bd.move_box([3, 1], [2, 0], 0, 0) == ([3, 1], [3, 1], [2, 0], [2, 0])  # a pin of both columns
    with pytest.raises(ValueError, match="max_move_n must be >= 0"):
        bd.move_box([3, 1], [2, 0], 1, -1)
    with pytest.raises(ValueError, match="n0"):
        bd.move_box([3, 1], [2], 1, 1)
    with pytest.raises(ValueError, match="max_move_n"):
        bd.move_box([3, 1], [2, 0], 1, [1])
    with pytest.raises(ValueError, match="not an integer"):
        bd.move_box([3, 1], [2, 0.5], 1, 1)


def test_bounds_arrays_layout_with_pairs_and_boxes(llama_online_model):
    model = llama_online_model
    fleets = [list(bc.devices(M, 0)) for M in (2, 3, 2, 4)]
    table = fleet_table(fleets, model)
    pairs = [None, ([1, 2, 3], None), ([1, 1], [5, 6]), None]
    got = bd.bounds_arrays(table, pairs)
    assert len(got) == 2  # no n list anywhere: the pair of arrays, as before
    assert got[0].tolist() == [0, 0, 1, 2, 3, 1, 1, 0, 0, 0, 0]
    assert got[1].tolist() == [IMAX] * 5 + [5, 6] + [IMAX] * 4
    mixed = [([1, 1], None, [-2, 1], None), ([1, 2, 3], None), None, (None, [9] * 4, None, [0, 2**40, -3, 5])]
    lo, hi, nlo, nhi = bd.bounds_arrays(table, mixed)
    assert all(a.dtype == np.int32 and a.shape == (11,) for a in (lo, hi, nlo, nhi))
    assert lo.tolist() == [1, 1, 1, 2, 3, 0, 0, 0, 0, 0, 0]
    assert hi.tolist() == [IMAX] * 7 + [9] * 4
    assert nlo.tolist() == [0, 1] + [0] * 9  # a negative n_min is "no bound"
    assert nhi.tolist() == [IMAX] * 7 + [0, IMAX, -3, 5]
    assert len(bd.bounds_arrays(table, [(None, None, None, None)] * 4)) == 2  # 4-tuples of None: no n arrays
    with pytest.raises(ValueError, match="n_max of 3 entries"):
        bd.bounds_arrays(table, [(None, None, None, [0, 0, 0]), None, None, None])
    with pytest.raises(ValueError, match="3 items"):
        bd.bounds_arrays(table, [(None, None, None), None, None, None])


def test_replacement_within_keeps_its_field_order():
    r = bd.ReplacementWithin(None, None, 0.0, 0, False, None, 0.0, 0, 0.0)
    assert r.moved_gpu_layers_within == 0
    assert bd.ReplacementWithin.__dataclass_fields__.keys().__reversed__().__next__() == "moved_gpu_layers_within"


# ------------------------------------------------------------------ the exact oracle against HiGHS
@pytest.mark.parametrize("M", [4, 16])
def test_exact_oracle_agrees_with_highs_on_the_n_caps(llama_online_model, M):
    """The kinds HiGHS was run on: "off" and "half" (seeds 0 .. 3, k = 1, 2, 4). Objective within 1e-9."""
    model = llama_online_model
    checked = skipped = 0
    for _, k, s, kind in xc.cases([M], [1, 2, 4], range(4), xc.CAP_KINDS):
        b = xc.box(model, M, k, s, kind)
        if b is None:  # the unbounded instance is infeasible: no case
            continue
        devs = bc.devices(M, s)
        st, x, _, obj, unique = xc.exact_answer(model, devs, k, b)
        p = xc.boxed_problem(model, devs, k, b)
        res = mo.highs_solve(p, mip_gap=1e-9)
        assert res.success == (st == 0), (M, k, s, kind)
        if st != 0:
            continue
        if not unique:
            skipped += 1
            continue
        checked += 1
        assert bc.rel(mo.objective_value(p, res.x), obj) <= 1e-9, (M, k, s, kind)
        assert (x[M:2 * M] <= np.asarray(b[3])).all(), (M, k, s, kind)
    assert checked >= 8 and skipped * 10 <= checked + skipped


def test_joint_boxes_are_feasible_unique_and_bind(llama_online_model):
    """Every joint-box case is feasible and unique; the n box changes the optimum of the w box alone in a good
    share of them (so the GPU tests on these cases test the n box)."""
    model = llama_online_model
    for M, k in ((4, 2), (16, 1), (24, 1)):
        changed = 0
        for s in range(12):
            for kind in xc.MOVE_KINDS:
                b = xc.box(model, M, k, s, kind)
                st, x, _, obj, unique = xc.exact_answer(model, bc.devices(M, s), k, b)
                assert st == 0 and unique, (M, k, s, kind)
                st2, _, _, _, obj2, _ = bc.exact_answer(model, bc.devices(M, s), k, b[0], b[1])
                assert st2 == 0 and obj2 <= obj + 1e-9 * max(1.0, abs(obj))
                changed += obj2 < obj - 1e-9 * max(1.0, abs(obj))
        assert changed >= 8, (M, k, changed)  # of 24


def test_crossing_and_gpuless_lower_bounds_are_infeasible(llama_online_model):
    model = llama_online_model
    seen = 0
    for M, k, s, kind in xc.cases([2, 4, 16], [1, 2], range(6), xc.BAD_KINDS):
        b = xc.box(model, M, k, s, kind)
        if b is None:
            continue
        seen += 1
        assert xc.exact_answer(model, bc.devices(M, s), k, b)[0] == 2, (M, k, s, kind)
    assert seen >= 60


# ------------------------------------------------------------------ pins against evaluate_plan_np
@pytest.mark.parametrize("M", [2, 4, 16, 24])
def test_pinned_boxes_price_the_plan(llama_online_model, M):
    """Both columns pinned to (w1, n1): the oracle is feasible exactly when evaluate_plan_np says the plan is, and
    the objectives agree within 1e-12."""
    model = llama_online_model
    feasible = 0
    for k in (k for k in (1, 2, 4) if int(model.L) // k >= M):  # W >= M: an incumbent exists
        for s in range(12):
            devs = bc.devices(M, s)
            w1, n1 = xc.incumbent(model, M, k, s)
            b = xc.box(model, M, k, s, "pin")
            assert (b[0], b[1], b[2], b[3]) == (list(w1), list(w1), list(n1), list(n1))
            st, x, _, obj, _ = xc.exact_answer(model, devs, k, b)
            ev = pl.evaluate_plan_np(fleet_table([list(devs)], model), model, 0, k, w1, n1, xc.KV)
            assert (st == 0) == (ev.status == 0), (M, k, s, st, ev)
            if st == 0:
                feasible += 1
                assert [int(round(v)) for v in x[:2 * M]] == list(w1) + list(n1)
                assert bc.rel(ev.obj_value, obj) <= 1e-12, (M, k, s)
    assert feasible >= 12


# ------------------------------------------------------------------ the CLI
def test_cli_parses_the_new_flags():
    p = cli._parser()
    a = p.parse_args(["--profile", "hermes_70b", "--evaluate-solution", "s.json", "--max-move", "2", "--max-move-n", "1"])
    assert (a.max_move, a.max_move_n, a.cpu_only) == (2, 1, None)
    a = p.parse_args(["--profile", "hermes_70b", "--cpu-only", "m3_air", "1"])
    assert a.cpu_only == ["m3_air", "1"] and a.max_move_n is None
    with pytest.raises(SystemExit):
        p.parse_args(["--profile", "hermes_70b", "--max-move-n", "one"])
    with pytest.raises(SystemExit):  # --max-move-n without --max-move
        cli.main(["--profile", "hermes_70b", "--evaluate-solution", "s.json", "--max-move-n", "1"])


def test_cpu_only_picks():
    class D:
        def __init__(self, name):
            self.name = name

    devs = [D("a"), D("b"), D("2")]
    assert cli.cpu_only_n_max(devs, ["b"]) == [IMAX, 0, IMAX]
    assert cli.cpu_only_n_max(devs, ["0", "2"]) == [0, IMAX, 0]  # "2" is a name first
    with pytest.raises(ValueError, match="neither"):
        cli.cpu_only_n_max(devs, ["3"])
    with pytest.raises(ValueError, match="neither"):
        cli.cpu_only_n_max(devs, ["c"])


def test_cli_cpu_only_solves_with_n_max_and_prints_the_usual_output(monkeypatch, capsys):
    from distilp_amd.solver.coefficients import HALDAResult

    from .helpers import fixture_fleet

    devs, model = fixture_fleet("hermes_70b")
    M = len(devs)
    w = [model.L // M + (1 if i < model.L % M else 0) for i in range(M)]
    result = HALDAResult(w=w, n=[0] * M, k=1, obj_value=12.5, sets={"M1": [], "M2": [], "M3": list(range(M))})
    calls = []

    def fake_bounded(devices, mdl, **kw):
        calls.append(kw)
        return result

    monkeypatch.setattr(cli, "halda_solve", lambda *a, **k: result)
    monkeypatch.setattr(bd, "halda_solve_bounded", fake_bounded)
    base = ["--profile", "hermes_70b", "--quiet", "--no-plot"]
    assert cli.main(base) == 0
    plain = capsys.readouterr().out
    assert not calls
    assert cli.main(base + ["--cpu-only", "0"]) == 0
    assert capsys.readouterr().out == plain  # the same result object: the same lines
    assert calls == [{"n_max": [0] + [IMAX] * (M - 1), "kv_bits": "4bit"}]
    assert cli.main(base + ["--cpu-only", "no-such-device"]) == 2


def test_within_line_with_an_n_budget(monkeypatch):
    from distilp_amd.solver.coefficients import HALDAResult

    got = HALDAResult(w=[3, 5], n=[0, 2], k=2, obj_value=1.25, sets={"M1": [], "M2": [], "M3": [0, 1]})
    seen = []

    def fake(fleets, model, boxes, ks, **kw):
        seen.append(boxes[0])
        return [got]

    monkeypatch.setattr(bd, "halda_solve_bounded_batch", fake)
    line = cli.within_line([None, None], None, (2, [4, 4], [1, 1]), 1, 1)
    assert line == "within 1 (n within 1): k=2, obj=1.250000, moved_layers=2, moved_gpu_layers=2"
    assert seen == [([3, 3], [5, 5], [0, 0], [2, 2])]
    assert cli.within_line([None, None], None, (2, [4, 4], [1, 1]), 1) == "within 1: k=2, obj=1.250000, moved_layers=2"
    assert seen[1] == ([3, 3], [5, 5])  # without the n budget: move_bounds' pair, as before
    monkeypatch.setattr(bd, "halda_solve_bounded_batch", lambda *a, **k: [None])
    assert cli.within_line([None, None], None, (2, [4, 4], [1, 1]), 1, 0) == "within 1 (n within 0): infeasible"
