"""Device selection and scale-in / scale-out on route "wide" (csrc/halda_rank.hpp: candidates carried as ranks)
at the smallest shapes the route can go wrong at: fleets of 65 and 70 devices whose droppable slots straddle the
64-device word and wave boundary, against the exact oracle and the enumeration over the entries behind it."""

import math

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import change as ch
from distilp_amd.solver import scale as sc
from distilp_amd.solver import subsets as ss
from distilp_amd.solver.subfleets import halda_solve_subfleets

from . import bounds_cases as bc
from . import change_cases as cc
from . import deep_cases as dc
from . import subsets_cases as sx

pytestmark = pytest.mark.gpu
KVB = "4bit"  # kv factor 0.5, bounds_cases.KV


def slots_of(M):
    return [0, 62, 63, 64, M - 1]


@pytest.mark.parametrize("M", [65, 70])
@pytest.mark.parametrize("max_drop", [1, 2])
def test_selection_equals_the_oracle_minimum(M, max_drop):
    """max_drop = 1: every device droppable; max_drop = 2: the five slots, 16 candidates."""
    key = ("deep", M, 0, bc.L, None)
    devs, model, kv, _ = sx.fleet_of(key)
    keep = () if max_drop == 1 else tuple(i for i in range(M) if i not in slots_of(M))
    pts = ss.halda_subset_frontier(devs, model, max_drop, keep, kv_bits=kv, route="wide")
    want = sx.brute_force_of(key, max_drop, keep)
    assert len(pts) == len(want) == max_drop + 1
    for d, (pt, (least, _, _)) in enumerate(zip(pts, want)):
        mine = sx.oracle_of(key, tuple(pt.kept))["obj_value"]
        print(M, max_drop, d, pt.dropped, pt.obj_value, least, mine)
        assert least < math.inf and len(pt.dropped) == d and not set(pt.dropped) & set(keep)
        assert bc.rel(pt.obj_value, least) <= sx.REL_OBJ and bc.rel(mine, least) <= sx.REL_OBJ
        assert pt.result == halda_solve_subfleets([devs], model, [(0, pt.kept)], kv_bits=kv)[0]


@pytest.mark.parametrize("L,k,slots,P", [(80, 1, (0, 62, 63, 64), 2), (160, 2, (0, 63, 64), 1)])
def test_scale_in_equals_the_enumerated_failover_minimum(llama_online_model, L, k, slots, P):
    M = 65
    model = dc.model_at(llama_online_model, L)
    devs, w = list(bc.devices(M, 0)), cc.parent(model, M, k, 100)[1]  # another seed's optimum: a stale incumbent
    inc = (k, w, [0] * M)
    keep = [i for i in range(M) if i not in slots]
    rows = sc.halda_scale_in_frontier(devs, model, inc, 2, P, keep=keep, kv_bits=KVB, route="wide")
    assert len(rows) == 3
    for d, row in enumerate(rows):
        lost = [c for c, _ in sx.candidates(M, keep, d)]
        frs = (ch.halda_failover_frontiers(devs, model, inc, P, lost, KVB, route="wide") if d else
               [ch.halda_change_frontier(devs, model, k, w, P, KVB, route="wide")])  # row 0: nothing is lost
        for p, pt in enumerate(row):
            best = min(range(len(lost)), key=lambda i: frs[i][p].obj_value)  # min keeps the earliest among equals
            assert pt.point == frs[best][p], (d, p, pt.dropped, lost[best])
            assert (pt.point.plan is None and pt.dropped == []) or pt.dropped == list(lost[best]), (d, p)
        _, listed, w0 = cc.lose(devs, w, tuple(row[P].dropped))
        want = cc.answer(model, listed, k, w0, (P,), "b", tag=(L, k, d))[P]
        print(L, k, d, row[P].dropped, row[P].point.obj_value, want)
        assert want is not None and bc.rel(row[P].point.obj_value, want) <= 1e-9


def test_scale_out_equals_the_enumeration_over_pool_subsets(llama_online_model):
    model, M, q, P = llama_online_model, 64, 3, 2
    every, w = list(bc.devices(M + q, 0)), cc.parent(llama_online_model, M, 1, 100)[1]
    devs, pool = every[:M], every[M:]
    fr = sc.halda_scale_out_frontier(devs, pool, model, (1, w, [0] * M), 2, P, KVB, route="wide")
    assert len(fr) == 3
    for a, row in enumerate(fr):
        adds = [tuple(j for j in range(q) if j not in out) for out, _ in sx.candidates(q, (), q - a)]  # left-out order
        frs = [ch.halda_change_frontier(devs + [pool[j] for j in add], model, 1, list(w) + [0] * a, P, KVB, route="wide")
               for add in adds]
        for p, pt in enumerate(row):
            best = min(range(len(adds)), key=lambda i: frs[i][p].obj_value)
            assert pt.point == frs[best][p], (a, p)
            assert pt.point.plan is None or pt.added == list(adds[best]), (a, p, pt.added)
    assert fr[1][P].point.plan is not None


@pytest.mark.parametrize("sizes", [(16,), (5, 16)])
def test_both_routes_agree_inside_the_wave_gate(llama_online_model, sizes):
    model = llama_online_model
    fleets = [list(bc.devices(M, 0)) for M in sizes]
    incs = [(1, cc.parent(model, M, 1, 100)[1], [0] * M) for M in sizes]
    assert ss.halda_subset_frontier_batch(fleets, model, 2, kv_bits=KVB, route="wide") == \
        ss.halda_subset_frontier_batch(fleets, model, 2, kv_bits=KVB)
    assert sc.halda_scale_in_frontier_batch(fleets, model, incs, 2, 2, kv_bits=KVB, route="wide") == \
        sc.halda_scale_in_frontier_batch(fleets, model, incs, 2, 2, kv_bits=KVB)
    # the raw grids: every array equal, objectives as uint64, the index lists against the masks
    from distilp_amd.solver.fleets import fleet_table

    table, w0 = fleet_table(fleets, model), np.concatenate([np.asarray(i[1], np.int32) for i in incs])
    wave = sc.solve_change_subsets_table(table, model, 1, w0, 0, 2, 2, bc.KV)
    wide = sc.solve_change_subsets_table(table, model, 1, w0, 0, 2, 2, bc.KV, route="wide")
    assert (wave.status == lh.STATUS_OPTIMAL).any()
    for f in ("status", "loaded", "released"):
        assert np.array_equal(getattr(wide, f), getattr(wave, f)), f
    assert np.array_equal(wide.obj.view(np.uint64), wave.obj.view(np.uint64))
    assert np.array_equal(wide.w[..., :64], wave.w) and np.array_equal(wide.n[..., :64], wave.n)
    assert not wide.w[..., 64:].any() and not wide.n[..., 64:].any()
    assert all(wide.gone(*c) == wave.gone(*c) for c in np.ndindex(wave.status.shape))
    sel_wave = ss.solve_subsets_table(table, model, [1, 2], bc.KV, 2, None)
    sel_wide = ss.solve_subsets_table(table, model, [1, 2], bc.KV, 2, None, route="wide")
    assert np.array_equal(sel_wide[0], sel_wave[0]) and np.array_equal(sel_wide[3], sel_wave[3])
    assert np.array_equal(sel_wide[1].view(np.uint64), sel_wave[1].view(np.uint64))
    assert all(sum(1 << int(i) for i in sel_wide[2][c] if i >= 0) == int(sel_wave[2][c]) for c in np.ndindex(sel_wave[2].shape))


def test_chunked_launches_equal_the_one_chunk_call(llama_online_model):
    model, M, P = llama_online_model, 65, 2
    from distilp_amd.solver.fleets import fleet_table

    table = fleet_table([list(bc.devices(M, 0))], model)
    w0 = np.asarray(cc.parent(model, M, 1, 100)[1], np.int32)
    one = sc.solve_change_subsets_table(table, model, 1, w0, 0, 1, P, bc.KV, route="wide")
    ctx = lh.get_context(0)
    top = sc.max_deficit(w0, list(range(M)), 1, int(model.L))
    cap = sc.launch_bytes_wide(M - 1, P, top, 1, 25)  # 25 of d = 1's 65 candidates per launch: three chunks
    assert sc.launch_bytes_wide(M - 1, P, top, 1, 65) > cap > sc.launch_bytes_wide(M - 1, P, top, 1, 22)
    sc.set_change_subsets_chunk(ctx, cap)
    try:
        cut = sc.solve_change_subsets_table(table, model, 1, w0, 0, 1, P, bc.KV, route="wide")
    finally:
        sc.set_change_subsets_chunk(ctx, 0)
    assert (one.status == lh.STATUS_OPTIMAL).any()
    for f in ("status", "dropped", "loaded", "released", "w", "n"):
        assert np.array_equal(getattr(cut, f), getattr(one, f)), f
    assert np.array_equal(cut.obj.view(np.uint64), one.obj.view(np.uint64))
