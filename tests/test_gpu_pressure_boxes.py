"""Many boxes on one table in ONE launch (halda_sweep_boxes_kernel, halda_sweep_boxes_tables_kernel) on the
memory-pressured, irregular and tight fleets of tests/pressure_box_cases.py, every slice against the exact oracle.
test_gpu_boxes.py meets the oracle on unscaled fleets only, where no box of a fleet is empty next to a feasible one
of the same fleet: here the planes of one call are ALL kinds at once, so every fleet has an empty box ("cross",
"nogpu", a "tcap" or "push" beyond what it holds) below and above feasible ones -- where a (box, fleet) item could
leak state into the next one. Status, objective within 1e-9, (w, n) inside the box, the full plan where the oracle's
uniqueness margin holds (test_gpu_pressure_box.check_against_oracle on every plane), None where the box is empty;
the loop test path gives the fused routes' bytes."""

from types import SimpleNamespace

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import boxes as bx
from distilp_amd.solver.fleets import fleet_table

from . import pressure_box_cases as pb
from . import pressure_cases as pc
from .test_gpu_pressure_box import check_against_oracle

pytestmark = pytest.mark.gpu

# one plane per kind of pb.KINDS: an always-empty kind first and another in the middle, so that every fleet has an
# empty box below a feasible one and a feasible one below an empty one
PLANES = ("cross", "box1", "box2", "off", "half", "pin", "nogpu", "push", "tcap")
assert sorted(PLANES) == sorted(pb.KINDS)
FIELDS = ("best_k", "obj_value", "w", "n", "obj_by_k", "status", "x")


@pytest.fixture
def ctx():
    c = lh.get_context(0)
    yield c
    bd.set_bounds_path(c, 0)
    bx.set_boxes_path(c, 0)


def boxes_of(fleets, k):
    """boxes[b][f]: the box of (fleet, k, PLANES[b]) as halda_solve_boxes_batch takes it, None where the fleet has
    no case of the kind."""
    return [[None if pb.box(f, k, kind) is None else tuple(list(a) for a in pb.box(f, k, kind)) for f in fleets]
            for kind in PLANES]


def assert_empty_and_feasible_boxes_interleave(fleets, k):
    """From the oracle's answers alone: some fleet has an empty box at a plane index BELOW a feasible one, and another
    fleet a feasible one below an empty one."""
    below, above = [], []
    for f in fleets:
        st = [None if pb.answer(f, k, kind) is None else pb.answer(f, k, kind)[1] for kind in PLANES]
        empty = [b for b, s in enumerate(st) if s is not None and s != 0]
        ok = [b for b, s in enumerate(st) if s == 0]
        if empty and ok and min(empty) < max(ok):
            below.append(f)
        if empty and ok and min(ok) < max(empty):
            above.append(f)
    assert below and above and len(set(below) | set(above)) >= 2, (k, below, above)
    return len(below), len(above)


def raw_planes(fleets, k, boxes):
    model = pc.our_model()
    table = fleet_table([pb.devices(f) for f in fleets], model)
    return table, bx.solve_boxes_table(table, model, [k], bx.box_planes(table, boxes), pc.kv_factor("4bit"))


def same_bytes(a, b, tag):
    for sa, sb in zip(a, b):
        for f in FIELDS:
            assert getattr(sa, f).tobytes() == getattr(sb, f).tobytes(), (tag, f)


def check_call(ctx, fleets, k, what, route=None):
    """One halda_solve_boxes_batch call and one raw call over `fleets` at k under every kind at once, against the
    oracle. Returns (route, the raw slices, the boxes)."""
    model = pc.our_model()
    assert all(pb.model_of(f) is model for f in fleets)
    boxes = boxes_of(fleets, k)
    n_below, n_above = assert_empty_and_feasible_boxes_interleave(fleets, k)
    out = bx.halda_solve_boxes_batch([pb.devices(f) for f in fleets], model, boxes, [k], kv_bits="4bit")
    took = bx.last_boxes_route(ctx)
    assert route is None or took == route, (what, took)
    table, raw = raw_planes(fleets, k, boxes)
    assert bx.last_boxes_route(ctx) == took
    off = [int(v) for v in table.dev_off]
    n_inst = feasible = compared = 0
    for b, kind in enumerate(PLANES):
        fs = raw[b]
        for M in sorted({f[1][0] for f in fleets}):
            at = [i for i, f in enumerate(fleets) if f[1][0] == M and boxes[b][i] is not None]
            if not at:
                continue
            N = 7 * M + 1
            got = {"status": fs.status[at, 0], "best_k": fs.best_k[at], "obj_value": fs.obj_value[at],
                   "obj_by_k": fs.obj_by_k[at, 0], "w": np.concatenate([fs.w[off[i]:off[i] + M] for i in at]),
                   "n": np.concatenate([fs.n[off[i]:off[i] + M] for i in at]),
                   "x": np.concatenate([fs.x[int(fs.x_off[i]):int(fs.x_off[i]) + N] for i in at])}
            assert all(int(fs.x_off[i]) >= 0 for i in at), (what, kind)
            inst = [(fleets[i], kind) for i in at]
            feasible += check_against_oracle(got, inst, SimpleNamespace(xs=N), M, k, f"{what} / {kind}")
            n_inst += len(inst)
            compared += sum(pb.answer(f, k, kind)[1] == 0 and pb.answer(f, k, kind)[5] for f, kind in inst)
        for i, f in enumerate(fleets):
            r, tag = out[b][i], (what, f, k, kind)
            if boxes[b][i] is None:  # no case of the kind: no bound, the free optimum
                st, x, _, _ = pb.exact(f, k)
                assert (r is None) == (st != 0), tag
                if r is not None:
                    obj = pc.objective(f[1], k) if f[0] == "p" else None
                    assert obj is None or pc.close(r.obj_value, obj), tag
                continue
            st, obj = pb.answer(f, k, kind)[1], pb.answer(f, k, kind)[4]
            assert (r is None) == (st != 0) == (fs.best_k[i] == 0), tag
            if r is not None:
                M = f[1][0]
                assert r.k == k and pc.close(r.obj_value, obj), tag + (r.obj_value, obj)
                assert r.w == fs.w[off[i]:off[i] + M].tolist() and r.n == fs.n[off[i]:off[i] + M].tolist(), tag
    print(f"{what}: route {took}, {len(fleets)} fleets x {len(PLANES)} planes, {n_inst} instances, {feasible} feasible,"
          " "
          f"{compared} plan compares; {n_below} fleets with an empty box below a feasible one, {n_above} the other way")
    # the plan is compared wherever the oracle's margin holds; outside the tie-heavy fleets that is 95 % or more
    clear = [(f, kind) for f in fleets if not pb.tie_heavy(f) for kind in PLANES
             if pb.answer(f, k, kind) is not None and pb.answer(f, k, kind)[1] == 0]
    assert feasible >= n_inst // 2 and sum(pb.answer(f, k, kind)[5] for f, kind in clear) >= 0.95 * len(clear) > 0, what
    return took, raw, boxes


def register_fleets(scale):
    return pb.pressured_fleets(64, scale) + [f for f in pb.tight_fleets(64) if f[1][1] == scale]


def mixed_fleets():
    """5-, 16- and 64-device pressured, irregular and tight fleets in one table, sizes interleaved."""
    out = []
    for s in (0, 1):
        out += [("p", (5, pc.S16, s, "4bit")), ("p", (64, pc.S16, s, "4bit")), ("p", (16, pc.S64, s, "4bit"))]
    out += pb.irregular_fleets(16)[:2] + pb.irregular_fleets(64)[:2]
    return out + [pb.tight_fleets(5)[0], pb.tight_fleets(64)[0], pb.tight_fleets(16)[0]]


# ------------------------------------------------------------------ 1. the register route
@pytest.mark.parametrize("scale", [pc.S16, pc.S64], ids=["1/16", "1/64"])
def test_every_kind_in_one_register_launch_equals_the_oracle(ctx, scale):
    took, raw, boxes = check_call(ctx, register_fleets(scale), 1, f"M = 64, 1/{scale.denominator}, k = 1", "register")
    if scale == pc.S64:  # the loop test path: the same bytes
        bx.set_boxes_path(ctx, 1)
        try:
            _, loop = raw_planes(register_fleets(scale), 1, boxes)
            assert bx.last_boxes_route(ctx) == "loop"
        finally:
            bx.set_boxes_path(ctx, 0)
        same_bytes(loop, raw, "register / loop")


# ------------------------------------------------------------------ 2. the table route
@pytest.mark.parametrize("M", [5, 16])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_every_kind_in_one_table_launch_equals_the_oracle(ctx, M, k):
    fleets = pb.fleets(M)
    took, raw, boxes = check_call(ctx, fleets, k, f"M = {M}, k = {k}", "tables")
    if (M, k) == (16, 2):
        bx.set_boxes_path(ctx, 1)
        try:
            _, loop = raw_planes(fleets, k, boxes)
            assert bx.last_boxes_route(ctx) == "loop"
        finally:
            bx.set_boxes_path(ctx, 0)
        same_bytes(loop, raw, "tables / loop")


# ------------------------------------------------------------------ 3. one mixed table
def test_a_mixed_table_of_5_16_and_64_device_fleets_equals_the_oracle(ctx):
    fleets = mixed_fleets()
    assert {f[0] for f in fleets} == {"p", "i", "t"} and {f[1][0] for f in fleets} == {5, 16, 64}
    took, _, _ = check_call(ctx, fleets, 1, "mixed 5 / 16 / 64, k = 1")
    assert took in ("register", "tables", "loop")
