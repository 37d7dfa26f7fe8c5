"""Route "wide" of the many-boxes entry on the GPU (halda_sweep_boxes_wide_kernel): HiGHS with the columns narrowed
at the widths where the workgroup's split can go wrong, the routes that exist inside their gates, the k-sweep and
its statuses, and the reload frontier of a fleet wider than a wave."""

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import boxes as bx
from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import fleet_table
from distilp_amd.solver.halda import halda_solve_batch
from oracle import milp_oracle as mo

from . import bounds_cases as bc
from . import box_cases as xc
from . import deep_cases as dc

gpu = pytest.mark.gpu
KVB = "4bit"  # kv factor 0.5, bounds_cases.KV
IMAX = xc.IMAX
# (M, L, k): lane = device with three idle waves; the last lane of wave 0 and the first of wave 1; one device in the
# third wave; every thread a device; the wide fleet at k > 1; R + 1 = 318 > 256 (two states a thread, rows in chunks)
SHAPES = [(3, 80, 1), (64, 160, 1), (65, 160, 1), (129, 160, 1), (256, 320, 1), (65, 160, 2), (3, 320, 1)]
KINDS = ("box1", "off", "half", "cross")


def _boxes(model, M, k):
    """box_cases' kinds of (M, k, seed 0), the unbounded box and n_max = 0 everywhere."""
    W = int(model.L) // k
    free = ([1] * M, [W] * M, [0] * M, [IMAX] * M)
    kinds = [xc.box(model, M, k, 0, kind) for kind in KINDS]
    return [b for b in kinds if b is not None] + [free, (*free[:3], [0] * M)]


@gpu
@pytest.mark.parametrize("M,L,k", SHAPES)
def test_wide_equals_highs_inside_every_box(llama_online_model, M, L, k):
    model = dc.model_at(llama_online_model, L)
    devs, W = list(bc.devices(M, 0)), L // k
    boxes = _boxes(model, M, k)
    table = fleet_table([devs], model)
    planes = bx.box_planes(table, [[b] for b in boxes])
    got = bx.solve_boxes_table(table, model, [k], planes, bc.KV, route="wide")
    plans = bx.halda_solve_boxes(devs, model, boxes, [k], KVB, route="wide")
    for b, box, res, r in zip(range(len(boxes)), boxes, got, plans):
        want = mo.highs_solve(xc.boxed_problem(model, devs, k, box), mip_gap=0.0)
        st = int(res.status[0, 0])
        assert st == (lh.STATUS_OPTIMAL if want.success else lh.STATUS_INFEASIBLE), (b, st)
        assert (r is None) == (not want.success) == (int(res.best_k[0]) == 0), b
        if r is None:
            assert not res.w.any() and not res.n.any() and res.obj_by_k[0, 0] == np.inf
            continue
        ref = mo.objective_value(xc.boxed_problem(model, devs, k, box), want.x)
        w, n = np.asarray(r.w), np.asarray(r.n)
        print(M, L, k, b, r.obj_value, ref)
        assert bc.rel(r.obj_value, ref) <= 1e-9, (b, r.obj_value, ref)
        assert w.sum() == W and (n <= w).all() and (w >= box[0]).all() and (w <= box[1]).all(), b
        assert (n >= box[2]).all() and (n <= box[3]).all(), b
        assert np.array_equal(w, res.w) and np.array_equal(n, res.n) and r.obj_value == res.obj_value[0]
        buf = pl.evaluate_table(table, model, np.full(1, k, np.int32), res.w, res.n, bc.KV)
        assert buf.status[0] == lh.STATUS_OPTIMAL, b
        assert res.obj_by_k[0:1, 0].view(np.uint64) == buf.obj.view(np.uint64), (b, res.obj_by_k[0, 0], buf.obj[0])
        pin = bd.halda_solve_bounded(devs, model, r.w, r.w, [k], KVB, n_min=r.n, n_max=r.n)
        assert bc.rel(pin.obj_value, r.obj_value) <= 1e-12, (b, pin.obj_value, r.obj_value)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.k == y.k and bc.rel(x.obj_value, y.obj_value) <= 1e-12, (x, y)


@gpu
def test_wide_equals_the_table_route_inside_its_gate(llama_online_model):
    model, ks = llama_online_model, [1, 2, 4, 5]
    fleets = [list(bc.devices(M, s)) for s, M in enumerate((1, 3, 7, 16, 16))]
    boxes = []
    for kind in ("box1", "box2", "off", "pin", "cross"):  # around each fleet's k = 2 incumbent
        boxes.append([xc.box(model, len(d), 2, s, kind) for s, d in enumerate(fleets)])
    boxes.append([None] * len(fleets))
    wide = bx.halda_solve_boxes_batch(fleets, model, boxes, ks, KVB, route="wide")
    tabs = bx.halda_solve_boxes_batch(fleets, model, boxes, ks, KVB)
    assert bx.last_boxes_route(lh.get_context(0)) == "tables"
    for a, b in zip(wide, tabs):
        _same(a, b)
    table = fleet_table(fleets, model)
    planes = bx.box_planes(table, boxes)
    for a, b in zip(bx.solve_boxes_table(table, model, ks, planes, bc.KV, route="wide"),
                    bx.solve_boxes_table(table, model, ks, planes, bc.KV)):
        assert np.array_equal(a.status, b.status) and np.array_equal(a.best_k, b.best_k)


@gpu
def test_wide_equals_the_loop_route_beyond_a_wave(llama_online_model):
    model = dc.model_at(llama_online_model, 160)
    fleets = [list(bc.devices(70, s)) for s in (0, 1)]
    inc = [bd.halda_solve_bounded(list(bc.devices(70, s + 100)), model, k_candidates=[1], kv_bits=KVB) for s in (0, 1)]
    boxes = [[bd.move_box(r.w, r.n, D, D) for r in inc] for D in (0, 1)] + [[None, None]]
    wide = bx.halda_solve_boxes_batch(fleets, model, boxes, [1], KVB, route="wide")
    loop = bx.halda_solve_boxes_batch(fleets, model, boxes, [1], KVB)
    assert bx.last_boxes_route(lh.get_context(0)) == "loop"
    for a, b in zip(wide, loop):
        _same(a, b)


@gpu
def test_k_sweep_and_statuses(llama_online_model):
    model = llama_online_model  # L = 80: its full k list
    devs = list(bc.devices(12, 3))
    ks = [d for d in range(1, 80) if 80 % d == 0]
    want = halda_solve_batch([devs], model, None, kv_bits=KVB)[0]
    got = bx.halda_solve_boxes(devs, model, [None, ([81] * 12, None)], None, KVB, route="wide")
    assert got[0].k == want.k and bc.rel(got[0].obj_value, want.obj_value) <= 1e-12
    assert got[1] is None  # sum w_min > W at every k
    table = fleet_table([devs], model)
    res = bx.solve_boxes_table(table, model, ks, bx.box_planes(table, [[None]]), bc.KV, route="wide")[0]
    small = np.asarray([80 // k >= 12 for k in ks])  # M > L // k: INFEASIBLE for that k only
    assert (res.status[0][small] == lh.STATUS_OPTIMAL).all() and (res.status[0][~small] == lh.STATUS_INFEASIBLE).all()
    assert np.isinf(res.obj_by_k[0][~small]).all() and res.best_k[0] == want.k


@gpu
def test_reload_frontier_of_a_70_device_fleet(llama_online_model):
    model = dc.model_at(llama_online_model, 160)
    devs = list(bc.devices(70, 0))
    old = bd.halda_solve_bounded(list(bc.devices(70, 100)), model, k_candidates=[1], kv_bits=KVB)
    pts = bx.halda_reload_frontier(devs, model, (1, old.w, old.n), max_points=6, kv_bits=KVB, route="wide")
    objs = [p.obj_value for p in pts]
    assert len(pts) == 6 and all(a >= b for a, b in zip(objs, objs[1:]))
    pinned = bd.halda_solve_bounded(devs, model, old.w, old.w, [1], KVB)
    assert bc.rel(objs[0], pinned.obj_value) <= 1e-12
    for p in pts:
        ref = bd.halda_solve_bounded(devs, model, None, [a + c for a, c in zip(old.w, p.caps)], [1], KVB,
                                     route="general")
        assert bc.rel(p.obj_value, ref.obj_value) <= 1e-12, (p.caps, p.obj_value, ref.obj_value)
