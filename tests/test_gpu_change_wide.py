"""The change frontier's workgroup route (halda_sweep_change_wide_kernel, route="wide"): the wave kernel's bits
inside the wave kernel's gate, and beyond it -- released budgets past the wave's LDS slice, lists wider than a
wave, a joiner on the last thread -- the free optimum, HiGHS with the release rows and the plan evaluation."""

import ctypes
import math
import types

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import budget as bg
from distilp_amd.solver import change as ch
from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import fleet_table
from distilp_amd.solver.subfleets import halda_solve_subfleets, pack_items

from . import bounds_cases as bc
from . import budget_cases as bu
from . import change_cases as cc
from . import deep_cases as dc
from .test_gpu_change import BEYOND_THE_GATE, KVB

gpu = pytest.mark.gpu
FIELDS = ("status", "loaded", "released", "w", "n")


def _raw(model, parents, items, k, w0s, P, route):
    table = fleet_table(parents, model)
    w0 = np.concatenate([np.asarray(w, np.int32) for w in w0s])
    return ch.solve_change_table(table, model, k, pack_items(table.sizes(), items), w0, P, bc.KV, route=route)


def _leave_one_out(parents_w):
    """(parents, items, w0s): every device of every (devs, w) parent lost in turn."""
    items, w0s = [], []
    for f, (devs, w) in enumerate(parents_w):
        for lost in range(len(devs)):
            keep, _, w0 = cc.lose(devs, w, lost)
            items.append((f, keep))
            w0s.append(w0)
    return [d for d, _ in parents_w], items, w0s


def _same_bits_shape(model, name):
    """(parents with their incumbents, k, P) of a shape both routes admit."""
    if name[0] == "B":
        k = int(name[-1])
        return [cc.parent(model, M, k, s) for M, kk, s in cc.LIST_B if kk == k], k, 4
    if name == "S_k1":
        return [cc.stale_parent(model, M, 1, s) for M, k, s in cc.LIST_S if k == 1], 1, 3
    if name == "W64":
        return [cc.parent(model, *cc.WIDE)], 1, 2
    fleets = [list(bc.devices(16, s)) for s in range(64)]  # 64 x 16: 1,024 items, more than the grid holds
    free = bd.halda_solve_bounded_batch(fleets, model, [None] * 64, [1], KVB)
    return [(d, r.w) for d, r in zip(fleets, free)], 1, 2


# ------------------------------------------------------------------ 1. inside the old gate: the wave kernel's bits
@gpu
@pytest.mark.parametrize("name", ["B_k1", "B_k2", "S_k1", "W64", "64x16"])
def test_wide_route_gives_the_wave_kernels_bits(llama_online_model, name):
    model = llama_online_model
    parents_w, k, P = _same_bits_shape(model, name)
    parents, items, w0s = _leave_one_out(parents_w)
    wave = _raw(model, parents, items, k, w0s, P, "wave")
    wide = _raw(model, parents, items, k, w0s, P, "wide")
    assert (wave.status == lh.STATUS_OPTIMAL).any()
    for f in FIELDS:
        assert np.array_equal(getattr(wide, f), getattr(wave, f)), (name, f)
    assert np.array_equal(wide.obj.view(np.uint64), wave.obj.view(np.uint64)), name


@gpu
def test_wide_route_with_no_deficit_is_the_budget_route(llama_online_model):
    model, (M, k, s), P = llama_online_model, bu.LIST_B[0], 4
    devs, w0 = list(bc.devices(M, s)), bu.golden()["B"][bu.key(M, k, s)]["w0"]
    got = _raw(model, [devs], [(0, list(range(M)))], k, [w0], P, "wide")
    want = bg.solve_budget_table(fleet_table([devs], model), model, k, np.asarray(w0, np.int32), P, bc.KV,
                                 route="wide")
    for f in ("status", "w", "n"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    assert np.array_equal(got.obj.view(np.uint64), want.obj.view(np.uint64))
    assert np.array_equal(got.loaded + got.released, want.moved) and np.array_equal(got.loaded, got.released)


# ------------------------------------------------------------------ 2. the far end the wave kernel cannot reach
@gpu
def test_wide_route_reaches_the_free_optimum_beyond_the_gate(llama_online_model):
    model, gold, P = llama_online_model, cc.golden()["S"], 72
    keys = sorted(BEYOND_THE_GATE["S"])
    assert len(keys) == 5 and all(BEYOND_THE_GATE["S"][c] == P for c in keys)
    parents, items, w0s = [], [], []
    for c in keys:
        M, k, s, lost = (int(v) for v in c.split(","))
        devs, w = cc.stale_parent(model, M, k, s)
        assert k == 1 and gold[c]["D"] == 1 and gold[c]["free_unique"]
        keep, _, w0 = cc.lose(devs, w, lost)
        parents.append(devs)
        items.append((len(items), keep))
        w0s.append(w0)
    wide = ch.halda_change_frontiers(parents, model, items, 1, w0s, P, KVB, route="wide")
    free = halda_solve_subfleets(parents, model, items, [1], kv_bits=KVB)
    for i, (c, fw, b) in enumerate(zip(keys, wide, free)):
        gp = cc.gate_p(ch, len(items[i][1]), 1, 1)
        wave = ch.halda_change_frontiers(parents, model, [items[i]], 1, [w0s[i]], gp, KVB)[0]
        print(c, gp, fw[P - 1].obj_value, fw[P].obj_value, b.obj_value)
        assert gp < P and len(fw) == P + 1
        assert bc.rel(fw[P].obj_value, b.obj_value) <= 1e-12, (c, fw[P].obj_value, b.obj_value)
        assert all(pt.obj_value == fw[P].obj_value for pt in fw[P:]), c
        assert fw[P - 1].obj_value > fw[P].obj_value, c  # unique optimum: one layer fewer is worse
        assert [pt.obj_value for pt in fw[:gp + 1]] == [pt.obj_value for pt in wave], c  # another route: same points


# ------------------------------------------------------------------ 3. wider than a wave
_STALE = {}


def _stale(base, M, k):
    """(model, devs, w) of the M-device fleet on the shallowest model that holds it, with the optimum of ANOTHER
    fleet as its incumbent (so that releases matter at k = 1)."""
    if (M, k) not in _STALE:
        model = dc.model_at(base, min(L for L in (160, 256, 320, 512) if L // k >= M + 4))
        w = bd.halda_solve_bounded(list(bc.devices(M, 100)), model, k_candidates=[k], kv_bits=KVB).w
        _STALE[M, k] = (model, list(bc.devices(M, 0)), [int(v) for v in w])
    return _STALE[M, k]


@gpu
@pytest.mark.parametrize("M,k,lost", [(66, 1, 0), (66, 1, 63), (66, 1, 64), (66, 1, 65), (66, 2, 0), (66, 2, 65),
                                      (70, 1, (3, 68)), (130, 1, 0), (130, 1, 129), (256, 1, 0), (256, 1, 255)])
def test_wide_lists_equal_highs_and_the_plan_evaluation(llama_online_model, M, k, lost):
    P = 2
    model, devs, w = _stale(llama_online_model, M, k)
    keep, listed, w0 = cc.lose(devs, w, lost)
    W, D = int(model.L) // k, int(model.L) // k - sum(w0)
    res = _raw(model, [devs], [(0, keep)], k, [w0], P, "wide")
    table, prob = fleet_table([listed], model), bu.problem(model, listed, k)
    assert (res.status == lh.STATUS_OPTIMAL).all()
    for p in range(P + 1):
        want, _ = cc.highs_change(prob, w0, p)
        buf = pl.evaluate_table(table, model, np.full(1, k, np.int32), res.w[p], res.n[p], bc.KV)
        print(M, k, lost, p, res.obj[0, p], want, buf.obj[0])
        assert bc.rel(res.obj[0, p], want) <= 1e-9, (p, res.obj[0, p], want)
        assert buf.status[0] == lh.STATUS_OPTIMAL and res.obj[0, p] == buf.obj[0], (p, res.obj[0, p], buf.obj[0])
        assert res.loaded[0, p] == D + res.released[0, p], p
        assert res.released[0, p] == np.maximum(0, np.asarray(w0) - res.w[p]).sum() <= p, p
        assert res.w[p].sum() == W, p


# ------------------------------------------------------------------ 4. a joiner in the last wave; mixed widths
@gpu
def test_a_joiner_on_the_last_thread(llama_online_model):
    model, devs, _ = _stale(llama_online_model, 256, 1)
    inc = bd.halda_solve_bounded(devs[:255], model, k_candidates=[1], kv_bits=KVB)
    fr = ch.halda_join_frontiers(devs[:255], devs[255:], model, (1, inc.w, inc.n), 2, KVB, route="wide")[0]
    assert fr[0].plan is None and fr[0].obj_value == math.inf
    prob, w0 = bu.problem(model, devs, 1), list(inc.w) + [0]
    for p in (1, 2):
        want, _ = cc.highs_change(prob, w0, p)
        print(p, fr[p].obj_value, want)
        assert fr[p].plan is not None and fr[p].plan.w[255] >= 1 and fr[p].released <= p
        assert bc.rel(fr[p].obj_value, want) <= 1e-9, (p, fr[p].obj_value, want)


@gpu
def test_mixed_widths_in_one_launch_equal_one_call_each(llama_online_model):
    model, devs, w = _stale(llama_online_model, 130, 1)
    items = [(0, s) for s in ([5, 64, 129], list(range(64)), list(range(65, 130)), list(range(1, 130)))]
    w0s = [[w[j] for j in s] for _, s in items]
    assert [len(s) for _, s in items] == [3, 64, 65, 129]
    one = ch.halda_change_frontiers([devs], model, items, 1, w0s, 2, KVB, route="wide")
    for it, w0, fr in zip(items, w0s, one):
        assert fr == ch.halda_change_frontiers([devs], model, [it], 1, [w0], 2, KVB, route="wide")[0], len(it[1])


# ------------------------------------------------------------------ 5. the gates and the routes (no GPU)
def test_wide_gate_and_its_figures():
    lib = lh.load_library()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    for M, P, D, k in ((1, 0, 0, 1), (4, 72, 1, 1), (70, 2, 9, 2), (256, 2, 250, 1), (256, 127, 0, 1)):
        assert lib.halda_change_wide_bytes(M, P, D, k, ctypes.byref(a), ctypes.byref(b)) == 0
        assert (a.value, b.value) == ch.change_wide_bytes(M, P, D, k), (M, P, D, k)
    assert lib.halda_change_wide_bytes(4, 3, -1, 1, ctypes.byref(a), ctypes.byref(b)) == -22
    assert ch.change_wide_bytes(4, 72, 1, 1)[0] >= 2 * 73 * 74 * 8 == 86432  # the planes of section 2's lists
    for k, D in ((1, 0), (2, 1)):
        first = next(P for P in range(ch.WIDE_MAX_P + 1) if ch.change_wide_bytes(16, P, D, k)[0] > ch.LDS_BUDGET)
        assert 90 <= first <= 100  # two planes of (P + 1)(D + P + 1) doubles in 160 KiB
        ch.check_gate_wide(ch.WIDE_MAX_DEVICES, 1, first - 1, D, k)
        with pytest.raises(ValueError):
            ch.check_gate_wide(16, 16, first, D, k)
    ch.check_gate_wide(256, 256, 2, 250, 1)
    for M, P, D in ((257, 3, 0), (16, 128, 0), (16, 2, 251), (16, 3, -1)):
        with pytest.raises(ValueError):
            ch.check_gate_wide(M, M, P, D, 1)


def test_routes_pick_their_entry(llama_online_model, monkeypatch):
    """"wave" raises where it always did; "auto" calls the wave entry inside check_gate and the wide one outside."""
    model, called = llama_online_model, []
    fake = types.SimpleNamespace(ctx=None, call=lambda name, *a: called.append(name))
    monkeypatch.setattr(ch, "get_context", lambda device=0: fake)
    W = int(model.L)
    for M, P, entry in ((16, 4, "halda_solve_change_host"), (16, 64, "halda_solve_change_wide_host"),
                        (65, 3, "halda_solve_change_wide_host")):
        table = fleet_table([list(bc.devices(M, 0))], model)
        items = pack_items(table.sizes(), [(0, list(range(M)))])
        w0 = np.asarray([W - M] + [1] * (M - 1), np.int32)  # a deficit of one layer
        ch.solve_change_table(table, model, 1, items, w0, P, bc.KV, route="auto")
        assert called.pop() == entry and not called
        if entry.endswith("wide_host"):
            for route in ("wave", None):  # None: the default
                with pytest.raises(ValueError):
                    ch.solve_change_table(table, model, 1, items, w0, P, bc.KV, **({"route": route} if route else {}))
            assert not called
    with pytest.raises(ValueError):
        ch.pick_route("tables", 16, 16, 4, 1, 1)
