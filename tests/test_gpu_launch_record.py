"""What a context remembers of its last launch, pinned per entry family ("The launch record").

Every single-launch entry of halda.hip leaves three things behind: the family's route (halda_last_<family>_route),
the kernels halda_last_fleet_ms names (or its HALDA_E_ARG where no timed launch stands), and the answer. Each case
here is one small call on a context created for it -- installed as the default context for the duration, since
the Python entries look that one up -- followed by asserts on all three; the answers are held to the exact
oracle through the helpers of tests/test_gpu_plan_edges.py on the cases of tests/plan_edge_cases.py.

The shapes are the smallest that reach each branch: two 4-device fleets on 7 layers with ks = [1, 2] (k = 2 has no
room: the register launch alone), fleets of 3 and 5 devices on 80 layers (k = 2 needs tables: the table launch
alone), and plan_edge_cases' two-device fleets at R + 1 = 64 / 65 for the families gated on the register launch
alone. The file states what the library did before its host side was folded into one launch record; it passed
unchanged on that build."""

import ctypes

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import boxes as bx
from distilp_amd.solver import halda_solve_variants
from distilp_amd.solver import plans as pl
from distilp_amd.solver import subfleets as sf
from distilp_amd.solver import variants as va
from distilp_amd.solver.fleets import fleet_table, solve_table

from . import plan_edge_cases as pe
from . import test_gpu_plan_edges as tpe

pytestmark = pytest.mark.gpu

REG_SHAPE = pe.Shape("rec_reg", "R", (4,), 7, (1, 2), pe._fl(4, (pe.ONE, 0), (pe.S16, 1)), {2: pe.REG}, None, None)
TAB_SHAPE = pe.Shape("rec_tab", "R", (3, 5), 80, (1, 2), ((3, pe.ONE, 0), (5, pe.S16, 1)), {2: pe.TABLES}, None, None)
REG2, TAB2 = "m2_r64", "m2_r65"  # two-device fleets, k = 1: the register launch alone / the table kernel alone
CSR = tpe.CSR_KERNELS | {"halda_pick_kernel"}
KV = pe.kv_factor(pe.KV)


@pytest.fixture
def ctx(monkeypatch):
    """A context of its own, timing on, standing in for the default context while the test runs."""
    c = lh.HaldaContext(0)
    monkeypatch.setitem(lh._contexts, 0, c)
    c.set_timing(True)
    yield c
    c.close()


def two(name):
    """(shape, model, cases, fleets): the first two fleets of a plan_edge_cases shape."""
    sh = pe.shape(name)
    cases = pe.cases_of(sh)[:2]
    return sh, pe.model_of(sh.L), cases, [pe.devices(c) for c in cases]


def record(ctx):
    """The kernels last_fleet_ms names, or None where it answers HALDA_E_ARG."""
    ms = (ctypes.c_double * 9)()
    rc = ctx.lib.halda_last_fleet_ms(ctx.ctx, ms)
    if rc != 0:
        assert rc == -22, rc
        return None
    return set(ctx.last_fleet_ms())


def same_record(ran, want):
    if want is CSR:
        assert "halda_lower_kernel" in ran and not (ran - CSR), ran
    else:
        assert ran == set(want), (ran, want)


# ------------------------------------------------------------------ the families: one oracle-checked call each
def fleets_call(ctx, sh):
    cases = pe.batch(sh, 2)
    model = pe.model_of(sh.L)
    table = fleet_table([pe.devices(c) for c in cases], model)
    res = solve_table(table, model, list(sh.ks), KV, want_x=True)
    tpe.check_sweep(cases, table, res, sh.name)


def subfleets_call(ctx, name=REG2):
    sh, model, cases, fleets = two(name)
    got = sf.halda_solve_subfleets(fleets, model, [(f, list(range(c[0]))) for f, c in enumerate(cases)],
                                   k_candidates=[1], kv_bits=pe.KV)
    for c, r in zip(cases, got):
        tpe.as_oracle(r, c, "sub-fleets")
    return sf.last_subfleets_route(ctx)


def variants_call(ctx, name=REG2):
    sh, model, cases, fleets = two(name)
    variants = [(model, "4bit"), (model, "8bit")]
    for (_, kv), rs in zip(variants, halda_solve_variants(fleets, variants, k_candidates=[1])):
        for c, r in zip(cases, rs):
            tpe.as_oracle(r, c[:4] + (kv,), f"variants {kv}")
    return va.last_variants_route(ctx)


def _oracle_plans(cases):
    out = []
    for c in cases:
        xo, M = pe.exact(c, 1)[1], c[0]
        out.append((1, [int(v) for v in np.rint(xo[:M])], [int(v) for v in np.rint(xo[M:2 * M])]))
    return out


def plans_call(ctx, name=REG2, ks=(1,)):
    sh, model, cases, fleets = two(name)
    table = fleet_table(fleets, model)
    k, w, n = pl._plan_arrays(table, _oracle_plans(cases), allow_none=False)
    res, buf = pl.solve_plans_table(table, model, list(ks), k, w, n, KV)
    for f, c in enumerate(cases):  # the oracle's optimum prices at the oracle's objective; the sweep finds it
        assert pe.close(float(buf.obj[f]), pe.objective(c, 1)), c
        off = int(res.x_off[f])
        assert res.status[f, 0] == lh.STATUS_OPTIMAL and res.best_k[f] == 1, c
        pe.check_x(res.x[off:off + 7 * c[0] + 1], c, 1, "plans")
        assert pe.close(float(res.obj_value[f]), pe.objective(c, 1)), c
    return pl.last_plans_route(ctx)


def bounds_call(ctx, name=REG2):
    sh, model, cases, fleets = two(name)
    boxes = tpe.move_boxes(cases, sh.L)
    got = bd.halda_solve_bounded_batch(fleets, model, boxes, k_candidates=[1], kv_bits=pe.KV)
    tpe.check_bounded(cases, boxes, got, "bounds")
    return bd.last_bounds_route(ctx)


def boxes_call(ctx, name=REG2):
    sh, model, cases, fleets = two(name)
    boxes = tpe.move_boxes(cases, sh.L)
    for row in bx.halda_solve_boxes_batch(fleets, model, [boxes, boxes], k_candidates=[1], kv_bits=pe.KV):
        tpe.check_bounded(cases, boxes, row, "boxes")
    return bx.last_boxes_route(ctx)


# ------------------------------------------------------------------ 1: halda_solve_fleets
@pytest.mark.parametrize("sh", [REG_SHAPE, TAB_SHAPE], ids=["register_alone", "tables_alone"])
def test_fleets_launch_is_named(ctx, sh):
    fleets_call(ctx, sh)
    assert record(ctx) == set(sh.launch[2])


# ------------------------------------------------------------------ 2: the forced paths and their automatic side
# (family, its call, the path set before it -- None: as created --, the shape, the route, the kernels named)
ROUTES = [
    ("subfleets", subfleets_call, None, REG2, "fused", pe.REG),
    ("subfleets", subfleets_call, 1, REG2, "expand", pe.REG),       # the expansion, then halda_solve_fleets
    ("variants", variants_call, None, REG2, "fused", pe.REG),
    ("variants", variants_call, None, TAB2, "fused", pe.TABLES),
    ("variants", variants_call, 1, REG2, "loop", pe.REG),
    ("plans", plans_call, 2, REG2, "fused", pe.REG),
    ("plans", plans_call, 2, TAB2, "two_launch", pe.TABLES),
    ("plans", plans_call, None, REG2, "two_launch", pe.REG),
    ("bounds", bounds_call, None, REG2, "fused", pe.REG),
    ("bounds", bounds_call, 1, REG2, "general", CSR),
    ("bounds", bounds_call, 3, TAB2, "tables", pe.TABLES),
    ("bounds", bounds_call, None, TAB2, "general", CSR),
    ("boxes", boxes_call, None, REG2, "register", pe.REG),
    ("boxes", boxes_call, None, TAB2, "tables", pe.TABLES),
    ("boxes", boxes_call, 1, REG2, "loop", pe.REG),                 # the boxed entry per box, under bounds path 3
    ("boxes", boxes_call, 1, TAB2, "loop", pe.TABLES),
]
ROUTE_IDS = [f"{f}-path{'_auto' if p is None else p}-{s}" for f, _, p, s, _, _ in ROUTES]


@pytest.mark.parametrize("family,call,path,shape,route,kernels", ROUTES, ids=ROUTE_IDS)
def test_route_and_launch_of_every_family(ctx, family, call, path, shape, route, kernels):
    if path is not None:
        lh.set_path(ctx, family, path)
    assert lh.last_route(ctx, family) == "none" and record(ctx) is None
    assert call(ctx, shape) == route
    same_record(record(ctx), kernels)
    if family == "boxes" and path == 1:  # the loop ran the boxed entry on the table route's path and put it back
        assert bd.last_bounds_route(ctx) == ("fused" if shape == REG2 else "tables")
        assert call(ctx, shape) == route and bounds_call(ctx, shape) == ("fused" if shape == REG2 else "general")


@pytest.mark.parametrize("family,call,path,shape,route,kernels", ROUTES, ids=ROUTE_IDS)
def test_an_untimed_call_leaves_no_record(ctx, family, call, path, shape, route, kernels):
    """With set_timing(False) every route still answers and names its route; last_fleet_ms fails, also where a
    timed call stood before it."""
    fleets_call(ctx, REG_SHAPE)
    assert record(ctx) == set(pe.REG)
    ctx.set_timing(False)
    if path is not None:
        lh.set_path(ctx, family, path)
    assert call(ctx, shape) == route
    assert record(ctx) is None


# ------------------------------------------------------------------ 3: the group launch, both persistent kinds
@pytest.mark.parametrize("name,nf,kernels", [(REG2, 2, pe.REG), ("one_slot", 66, pe.KSLOT)],
                         ids=["steps", "kslot_steps"])
@pytest.mark.parametrize("timed", [True, False])
def test_group_launch_of_two_plans_and_two_steps(ctx, name, nf, kernels, timed):
    import torch

    from distilp_amd.solver.fleets import DeviceFleetTable, PlanGroup

    sh = pe.shape(name)
    model, cases = pe.model_of(sh.L), pe.batch(sh, nf)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    sets = [cases, cases[::-1]]
    tabs = []
    for cs in sets:
        table = fleet_table([pe.devices(c) for c in cs], model)
        tabs.append((table, DeviceFleetTable(table, model, list(sh.ks), KV, dev, want_per_k=True)))
    group = PlanGroup([dt for _, dt in tabs], ctx)
    try:
        assert group.persistent
        for _, dt in tabs:
            for v in dt.out.values():
                v.zero_()
        torch.cuda.synchronize(dev)
        ctx.set_timing(timed)
        group.launch(0, 2, stream.cuda_stream)
        torch.cuda.synchronize(dev)
        assert record(ctx) == (set(kernels) if timed else None)
        for cs, (table, dt) in zip(sets, tabs):
            tpe.check_resident(cs, table, dt, list(sh.ks), f"group {name}")
    finally:
        group.close()


# ------------------------------------------------------------------ 4: the fused subsets route
def test_fused_subsets_leave_no_timed_record(ctx, llama_online_model):
    """halda_solve_subsets' fused launches record no events and clear the timed flag: last_fleet_ms fails after
    them, with timing on and a timed sweep before. The frontier against the enumerated candidates
    (test_gpu_subsets.check_frontier)."""
    from . import test_gpu_subsets as tss

    fleets_call(ctx, TAB_SHAPE)
    assert record(ctx) == set(pe.TABLES)
    devs = tss.fleet(64, 4300)
    out = tss.solve_subsets_device(fleet_table([devs], llama_online_model), llama_online_model, 1)
    assert out[4] == "fused" and record(ctx) is None
    assert lh.last_route(ctx, "subfleets") == "none"
    again = tss.check_frontier([devs], llama_online_model, 1, paths=(0,), sample=16, route0="fused")
    for a, b in zip(out[:4], again):
        assert a.tobytes() == b.tobytes()


def test_expanded_subsets_keep_the_subfleets_knobs(ctx, llama_online_model):
    """The expansion route forces the sub-fleet entry onto its own expansion and puts that entry's path and route
    back: afterwards the sub-fleet route still reads "none" and an automatic sub-fleet call is fused. The timed
    record is that of the expansion's last halda_solve_fleets launch (one-device lists, k > 1: the table kernel)."""
    from . import test_gpu_subsets as tss

    devs = tss.fleet(3, 11)
    out = tss.solve_subsets_device(fleet_table([devs], llama_online_model), llama_online_model, 2, path=1)
    assert out[4] == "expand" and lh.last_route(ctx, "subfleets") == "none"
    assert record(ctx) == set(pe.TABLES)
    assert subfleets_call(ctx) == "fused"
    again = tss.check_frontier([devs], llama_online_model, 2, paths=(1,))
    for a, b in zip(out[:4], again):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 5: an argument error after a timed call
def _bad_fleets(ctx, table, model, cases, sh):
    solve_table(table, model, [2, 1], KV, want_x=True)


def _bad_subfleets(ctx, table, model, cases, sh):
    parent, sub_off, sub_idx = sf.pack_items(table.sizes(), [(f, list(range(c[0]))) for f, c in enumerate(cases)])
    sf.solve_items(table, parent, sub_off, sub_idx, model, [2, 1], KV, 0, None)


def _bad_variants(ctx, table, model, cases, sh):
    va.solve_variants_table(table, [(model, "4bit"), (model, "8bit")], [2, 1])


def _bad_plans(ctx, table, model, cases, sh):
    k, w, n = pl._plan_arrays(table, _oracle_plans(cases), allow_none=False)
    pl.solve_plans_table(table, model, [2, 1], k, w, n, KV)


def _bad_bounds(ctx, table, model, cases, sh):
    lo, hi = bd.bounds_arrays(table, tpe.move_boxes(cases, sh.L))[:2]
    bd.solve_bounded_table(table, model, [2, 1], lo, hi, KV)


def _bad_boxes(ctx, table, model, cases, sh):
    boxes = tpe.move_boxes(cases, sh.L)
    bx.solve_boxes_table(table, model, [2, 1], bx.box_planes(table, [boxes, boxes]), KV)


ERRORS = [("fleets", None, _bad_fleets), ("subfleets", subfleets_call, _bad_subfleets),
          ("variants", variants_call, _bad_variants), ("plans", plans_call, _bad_plans),
          ("bounds", bounds_call, _bad_bounds), ("boxes", boxes_call, _bad_boxes)]


@pytest.mark.parametrize("family,call,bad", ERRORS, ids=[e[0] for e in ERRORS])
def test_a_rejected_call_leaves_the_record_and_the_route(ctx, family, call, bad):
    """A timed table launch by the family's own entry (halda_solve_fleets for the family without a route), then a
    call of the same entry with a descending k list, which the argument check rejects before any launch: the
    record and the route are those of the call before, and the next launch is named as usual."""
    sh, model, cases, fleets = two(TAB2)
    if family == "plans":
        lh.set_path(ctx, family, 2)
    if call is None:
        fleets_call(ctx, TAB_SHAPE)
        route = None
    else:
        route = call(ctx, TAB2)
    before = record(ctx)
    assert before is not None
    table = fleet_table(fleets, model)
    with pytest.raises(RuntimeError, match="ascending"):
        bad(ctx, table, model, cases, sh)
    assert record(ctx) == before
    if call is not None:
        assert lh.last_route(ctx, family) == route
    fleets_call(ctx, REG_SHAPE)
    assert record(ctx) == set(pe.REG)
    if call is not None:
        assert lh.last_route(ctx, family) == route
