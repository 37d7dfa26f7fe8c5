"""Per-device layer bounds without a GPU: the oracle of the bounded instances (the exact solver against HiGHS),
move_bounds, the argument checks, the C struct and exports, the CLI flag, and the new kernel's code object."""

import ctypes
import re

import numpy as np
import pytest

from distilp_amd.cli import solver as cli
from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver.fleets import HaldaBoundsC, fleet_table
from oracle import milp_oracle as mo

from . import bounds_cases as bc
from .conftest import REPO
from .test_abi import kernel_resources


# ------------------------------------------------------------------ the oracle of the bounded instances
@pytest.mark.parametrize("M", [4, 8])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_exact_oracle_and_highs_agree_on_bounded_instances(llama_online_model, M, k):
    model = llama_online_model
    differ = 0
    for _, _, s, D in bc.cases([M], [k], kinds=(1, 2)):
        devs = bc.devices(M, s)
        lo, hi = bc.box(model, M, k, s, D)
        st, w, n, cx, obj, unique = bc.exact_answer(model, devs, k, lo, hi)
        assert st == 0 and unique, (M, k, s, D)  # feasible and unique: no case is skipped
        p = bc.bounded_problem(model, devs, k, lo, hi)
        res = mo.highs_solve(p, mip_gap=1e-4)
        assert res.success, (M, k, s, D)
        hw = [int(round(v)) for v in res.x[:M]]
        hn = [int(round(v)) for v in res.x[M:2 * M]]
        assert (hw, hn) == (w, n), (M, k, s, D)
        assert bc.rel(mo.objective_value(p, res.x), obj) <= 1e-9, (M, k, s, D)
        free = mo.exact_solve(mo.lower_dense(list(devs), model, k, bc.KV))[1]
        differ += [int(round(v)) for v in free[:M]] != w
    assert differ >= 18  # of 24: the boxes bind


# ------------------------------------------------------------------ move_bounds and the argument checks
def test_move_bounds():
    assert bd.move_bounds([3, 1, 5], 2) == ([1, 1, 3], [5, 3, 7])
    assert bd.move_bounds([3, 1, 5], [0, 1, 4]) == ([3, 1, 1], [3, 2, 9])
    assert bd.move_bounds(np.asarray([2, 2]), np.int64(0)) == ([2, 2], [2, 2])
    for bad in (-1, [1, 2], [1, 1, -1], 1.5, [1, 1, 1.0]):
        with pytest.raises(ValueError):
            bd.move_bounds([3, 1, 5], bad)


def test_argument_validation():
    assert bd.check_bounds(None, None, 3) == (None, None)
    assert bd.check_bounds([1, 2, 3], (9, 1, 3), 3) == ([1, 2, 3], [9, 1, 3])  # w_max < w_min is not an error
    for w_min, w_max in (([1, 1], None), (None, [1, 1, 1, 1]), ([1, 1.5, 1], None), (None, [1, "2", 3]),
                         ([0, 1, 1], None), ([1, -2, 1], None), ([1, True, 1], None)):
        with pytest.raises(ValueError):
            bd.check_bounds(w_min, w_max, 3)


def test_batch_entries_check_their_arguments_before_any_gpu_call(llama_online_model):
    devs = list(bc.devices(4, 0))
    with pytest.raises(ValueError, match="bounds for"):
        bd.halda_solve_bounded_batch([devs], llama_online_model, [])
    with pytest.raises(ValueError, match="w_min"):
        bd.halda_solve_bounded_batch([devs], llama_online_model, [([1, 1, 1], None)])
    with pytest.raises(ValueError, match=">= 1"):
        bd.halda_solve_bounded(devs, llama_online_model, w_min=[0, 1, 1, 1])
    with pytest.raises(ValueError, match="not an integer"):
        bd.halda_solve_bounded(devs, llama_online_model, w_max=[1, 2.0, 1, 1])


def test_bounds_arrays_layout(llama_online_model):
    table = fleet_table([list(bc.devices(4, 0)), list(bc.devices(8, 1)), list(bc.devices(4, 2))], llama_online_model)
    lo, hi = bd.bounds_arrays(table, [None, ([2] * 8, None), (None, [5, 2**40, 7, 8])])
    assert lo.dtype == np.int32 and hi.dtype == np.int32
    assert lo.tolist() == [0] * 4 + [2] * 8 + [0] * 4
    assert hi.tolist() == [bd.INT32_MAX] * 12 + [5, bd.INT32_MAX, 7, 8]


# ------------------------------------------------------------------ the C surface
def test_bounds_struct_layout_matches_the_header():
    text = (REPO / "include" / "halda.h").read_text()
    m = re.search(r"typedef struct halda_bounds \{(.*?)\} halda_bounds;", text, re.S)
    assert m and re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split() == ["const", "int32_t", "*w_min,", "*w_max;"]
    assert [f[0] for f in HaldaBoundsC._fields_] == ["w_min", "w_max"]
    assert HaldaBoundsC.w_min.offset == 0 and HaldaBoundsC.w_max.offset == 8 and ctypes.sizeof(HaldaBoundsC) == 16
    assert "#define HALDA_ABI_VERSION 3" in text


NEW = ("halda_solve_fleets_bounded", "halda_solve_fleets_bounded_host", "halda_last_bounds_route",
       "halda_set_bounds_path")


def test_binding_exports_the_new_symbols():
    raw = ctypes.CDLL(str(lh.LIB_PATH))
    for name in NEW:
        assert name in lh.EXPORTS and hasattr(raw, name), name
    raw.halda_set_bounds_path.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert raw.halda_set_bounds_path(None, 1) == -22
    raw.halda_last_bounds_route.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert raw.halda_last_bounds_route(None, None) == -22
    import distilp.solver as alias
    import distilp_amd.solver as pkg

    for name in ("halda_solve_bounded", "halda_solve_bounded_batch", "move_bounds", "halda_replace_within"):
        assert getattr(alias, name) is getattr(pkg, name) is getattr(bd, name)


def test_new_kernel_uses_no_scratch_and_spills_no_vgpr(tmp_path):
    res = kernel_resources(tmp_path)
    for name in ("halda_sweep_bounds_kernel", "halda_bound_cols_kernel"):
        r = res[name]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
    assert res["halda_sweep_bounds_kernel"]["vgpr_count"] <= 128  # four waves per SIMD, as the sweep kernel


# ------------------------------------------------------------------ the CLI
def test_cli_parses_max_move():
    p = cli._parser()
    a = p.parse_args(["--profile", "hermes_70b", "--evaluate-solution", "s.json", "--max-move", "2"])
    assert a.max_move == 2 and a.evaluate_solution == "s.json"
    assert p.parse_args(["--profile", "hermes_70b"]).max_move is None
    with pytest.raises(SystemExit):
        p.parse_args(["--profile", "hermes_70b", "--max-move", "two"])
    with pytest.raises(SystemExit):  # needs the plan to move away from
        cli.main(["--profile", "hermes_70b", "--max-move", "2"])


def test_cli_output_is_unchanged_without_max_move(monkeypatch, capsys, tmp_path):
    """main() with and without --max-move on a stubbed solver: the same lines, plus the `within` line last."""
    from .helpers import fixture_fleet

    devs, model = fixture_fleet("hermes_70b")
    from distilp_amd.solver.coefficients import HALDAResult
    from distilp_amd.solver.plans import PlanEvaluation

    M = len(devs)
    w = [model.L // M + (1 if i < model.L % M else 0) for i in range(M)]
    result = HALDAResult(w=w, n=[0] * M, k=1, obj_value=12.5, sets={"M1": [], "M2": [], "M3": list(range(M))})
    monkeypatch.setattr(cli, "halda_solve", lambda *a, **k: result)
    monkeypatch.setattr(cli, "halda_evaluate_plan", lambda *a, **k: PlanEvaluation(True, 13.0, 1.0, 0))
    calls = []

    def fake_within(devices, mdl, plan, D):
        calls.append((plan, D))
        return f"within {D}: k=1, obj=12.750000, moved_layers=2"

    monkeypatch.setattr(cli, "within_line", fake_within)
    sol = tmp_path / "sol.json"
    base = ["--profile", "hermes_70b", "--quiet", "--no-plot"]
    assert cli.main(base + ["--save-solution", str(sol)]) == 0
    capsys.readouterr()
    assert cli.main(base + ["--evaluate-solution", str(sol)]) == 0
    plain = capsys.readouterr().out
    assert not calls and "within" not in plain
    assert cli.main(base + ["--evaluate-solution", str(sol), "--max-move", "2"]) == 0
    moved = capsys.readouterr().out
    assert moved == plain + "within 2: k=1, obj=12.750000, moved_layers=2\n"
    assert calls == [((1, w, [0] * M), 2)]


def test_within_line_formats(monkeypatch):
    from distilp_amd.solver.coefficients import HALDAResult

    got = HALDAResult(w=[3, 5], n=[0, 1], k=2, obj_value=1.25, sets={"M1": [], "M2": [], "M3": [0, 1]})
    monkeypatch.setattr(bd, "halda_solve_bounded_batch", lambda *a, **k: [got])
    assert cli.within_line([None, None], None, (2, [4, 4], [0, 0]), 1) == "within 1: k=2, obj=1.250000, moved_layers=2"
    monkeypatch.setattr(bd, "halda_solve_bounded_batch", lambda *a, **k: [None])
    assert cli.within_line([None, None], None, (2, [4, 4], [0, 0]), 1) == "within 1: infeasible"
