"""The move budget's workgroup route (halda_sweep_budget_wide_kernel, route="wide"): the wave kernel's bits inside
the wave kernel's gate, and beyond it -- budgets past the wave's LDS slice, fleets wider than a wave -- the free
optimum, HiGHS with the budget rows, the pinned bounded solve and the plan evaluation."""

import ctypes
import types

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import budget as bg
from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import fleet_table

from . import bounds_cases as bc
from . import budget_cases as bu
from . import deep_cases as dc
from .test_gpu_budget import BEYOND_THE_GATE, KVB, gate_p

gpu = pytest.mark.gpu


def _list_b(model, k, seeds=range(6)):
    gold = bu.golden()["B"]
    return [list(bc.devices(16, s)) for s in seeds], [gold[bu.key(16, k, s)]["w0"] for s in seeds]


def _same_bits_shape(model, name):
    """(fleets, w0s, k, P) of a shape both routes admit."""
    if name.startswith("B16"):
        k = int(name[-1])
        return (*_list_b(model, k), k, 4)
    if name == "A3+4":
        gold, cases = bu.golden()["A"], [c for c in bu.LIST_A if c[1] == 2]
        return [list(bc.devices(M, s)) for M, _, s in cases], [gold[bu.key(*c)]["w0"] for c in cases], 2, 3
    devs, w0 = bu.list_case(model, 64, 1, 0)
    return [devs], [w0], 1, 2


# ------------------------------------------------------------------ 1. inside the old gate: the wave kernel's bits
@gpu
@pytest.mark.parametrize("name", ["B16k1", "B16k2", "B16k4", "A3+4", "one64"])
def test_wide_route_gives_the_wave_kernels_bits(llama_online_model, name):
    model = llama_online_model
    fleets, w0s, k, P = _same_bits_shape(model, name)
    table, w0 = fleet_table(fleets, model), np.concatenate([np.asarray(w, np.int32) for w in w0s])
    wave = bg.solve_budget_table(table, model, k, w0, P, bc.KV, route="wave")
    wide = bg.solve_budget_table(table, model, k, w0, P, bc.KV, route="wide")
    assert (wave.status == lh.STATUS_OPTIMAL).all()
    for f in ("status", "moved", "w", "n"):
        assert np.array_equal(getattr(wide, f), getattr(wave, f)), (name, f)
    assert np.array_equal(wide.obj.view(np.uint64), wave.obj.view(np.uint64)), name


# ------------------------------------------------------------------ 2. the far end the wave kernel cannot reach
BEYOND = {c: p for cases in BEYOND_THE_GATE.values() for c, p in cases.items()}


@gpu
@pytest.mark.parametrize("M,k", sorted({c[:2] for c in BEYOND}))
def test_wide_route_reaches_the_free_optimum_beyond_the_gate(llama_online_model, M, k):
    model = llama_online_model
    sub = [c for c in BEYOND if c[:2] == (M, k)]
    gold = bu.golden()["A" if M < 8 else "B"]
    fleets = [list(bc.devices(M, s)) for _, _, s in sub]
    incs = [(k, gold[bu.key(*c)]["w0"], [0] * M) for c in sub]
    P, gp = max(BEYOND[c] for c in sub), gate_p(M, k)
    wide = bg.halda_move_frontier_batch(fleets, model, incs, 2 * P, KVB, route="wide")
    wave = bg.halda_move_frontier_batch(fleets, model, incs, 2 * gp, KVB)
    free = bd.halda_solve_bounded_batch(fleets, model, [None] * len(sub), [k], KVB)
    for c, fw, fv, b in zip(sub, wide, wave, free):
        ps = BEYOND[c]
        assert gp < ps <= P and len(fw) == P + 1
        print(c, ps, fw[ps - 1].obj_value, fw[ps].obj_value, b.obj_value)
        assert bc.rel(fw[ps].obj_value, b.obj_value) <= 1e-12, (c, fw[ps].obj_value, b.obj_value)
        assert all(pt.obj_value == fw[ps].obj_value for pt in fw[ps:]), c
        assert fw[ps - 1].obj_value > fw[ps].obj_value, c  # unique optimum: one layer fewer is worse
        assert [pt.obj_value for pt in fw[:gp + 1]] == [pt.obj_value for pt in fv], c  # another route: same points


# ------------------------------------------------------------------ 3. just past the LDS gate at k > 1
@gpu
def test_wide_route_one_point_past_the_wave_gate_at_k2(llama_online_model):
    model, k = llama_online_model, 2
    gp = gate_p(16, k)
    assert gp == 45
    fleets, w0s = _list_b(model, k, (0, 1))
    incs = [(k, w0, [0] * 16) for w0 in w0s]
    wide = bg.halda_move_frontier_batch(fleets, model, incs, 2 * (gp + 1), KVB, route="wide")
    wave = bg.halda_move_frontier_batch(fleets, model, incs, 2 * gp, KVB)
    for devs, w0, fw, fv in zip(fleets, w0s, wide, wave):
        assert [pt.obj_value for pt in fw[:gp + 1]] == [pt.obj_value for pt in fv]
        want, _ = bu.highs_budget(bu.problem(model, devs, k), w0, gp + 1)
        print(fw[gp + 1].obj_value, want)
        assert bc.rel(fw[gp + 1].obj_value, want) <= 1e-9, (fw[gp + 1].obj_value, want)


# ------------------------------------------------------------------ 4. wider than a wave
@gpu
@pytest.mark.parametrize("M,k", [(65, 1), (70, 1), (129, 1), (256, 1), (65, 2)])
def test_wide_fleets_equal_highs_the_pinned_solve_and_the_plan_evaluation(llama_online_model, M, k):
    P = 3
    model = dc.model_at(llama_online_model, min(L for L in (160, 256, 320, 512) if L // k >= M + 4))
    devs = list(bc.devices(M, 0))
    w0 = bd.halda_solve_bounded(list(bc.devices(M, 100)), model, k_candidates=[k], kv_bits=KVB).w
    table = fleet_table([devs], model)
    res = bg.solve_budget_table(table, model, k, np.asarray(w0, np.int32), P, bc.KV, route="wide")
    pinned = bd.halda_solve_bounded_batch([devs], model, [(w0, w0)], [k], KVB)[0]
    prob = bu.problem(model, devs, k)
    assert (res.status == lh.STATUS_OPTIMAL).all()
    for p in range(P + 1):
        want, _ = bu.highs_budget(prob, w0, p)
        buf = pl.evaluate_table(table, model, np.full(1, k, np.int32), res.w[p], res.n[p], bc.KV)
        print(M, k, p, res.obj[0, p], want, buf.obj[0])
        assert bc.rel(res.obj[0, p], want) <= 1e-9, (p, res.obj[0, p], want)
        assert buf.status[0] == lh.STATUS_OPTIMAL and res.obj[0, p] == buf.obj[0], (p, res.obj[0, p], buf.obj[0])
        assert res.moved[0, p] == np.abs(res.w[p] - np.asarray(w0)).sum() <= 2 * p, p
    assert bc.rel(res.obj[0, 0], pinned.obj_value) <= 1e-12, (res.obj[0, 0], pinned.obj_value)


# ------------------------------------------------------------------ 5. the gates (no GPU)
def test_wide_gate_and_its_figures():
    lib = lh.load_library()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    for M, P, k in ((1, 0, 1), (16, 46, 2), (70, 3, 1), (256, 98, 1), (256, 127, 4)):
        assert lib.halda_budget_wide_bytes(M, P, k, ctypes.byref(a), ctypes.byref(b)) == 0
        assert (a.value, b.value) == bg.budget_wide_bytes(M, P, k), (M, P, k)
    assert lib.halda_budget_wide_bytes(0, 1, 1, ctypes.byref(a), ctypes.byref(b)) == -22
    for k in (1, 2):
        first = next(P for P in range(bg.WIDE_MAX_P + 1) if bg.budget_wide_bytes(16, P, k)[0] > bg.LDS_BUDGET)
        assert 90 <= first <= 100  # two planes of (P + 1)^2 doubles in 160 KiB
        bg.check_gate_wide(16, 16, first - 1, k)
        bg.check_gate_wide(bg.WIDE_MAX_DEVICES, 1, first - 1, k)
        with pytest.raises(ValueError):
            bg.check_gate_wide(16, 16, first, k)
    for M, P in ((257, 3), (16, 128)):
        with pytest.raises(ValueError):
            bg.check_gate_wide(M, M, P, 1)


def test_routes_pick_their_entry(llama_online_model, monkeypatch):
    """"wave" raises where it always did; "auto" calls the wave entry inside check_gate and the wide one outside."""
    model, called = llama_online_model, []
    fake = types.SimpleNamespace(ctx=None, call=lambda name, *a: called.append(name))
    monkeypatch.setattr(bg, "get_context", lambda device=0: fake)
    W = int(model.L)
    for M, P, entry in ((16, 4, "halda_solve_fleets_budget_host"), (16, 48, "halda_solve_fleets_budget_wide_host"),
                        (65, 3, "halda_solve_fleets_budget_wide_host")):
        table = fleet_table([list(bc.devices(M, 0))], model)
        w0 = np.asarray([W - M + 1] + [1] * (M - 1), np.int32)
        bg.solve_budget_table(table, model, 1, w0, P, bc.KV, route="auto")
        assert called.pop() == entry and not called
        if entry.endswith("wide_host"):
            for route in ("wave", None):  # None: the default
                with pytest.raises(ValueError):
                    bg.solve_budget_table(table, model, 1, w0, P, bc.KV, **({"route": route} if route else {}))
            assert not called
    with pytest.raises(ValueError):
        bg.pick_route("tables", 16, 16, 4, 1)
