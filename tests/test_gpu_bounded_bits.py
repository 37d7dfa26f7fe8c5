"""The bounded sweep's fused kernels pinned bit for bit under BINDING bounds (tests/golden/bounded_bits.npz,
recorded by tests/golden/gen_bounded_bits.py): every call of CALLS is replayed and the raw bytes of the eight
outputs of Run.collect() -- best_k, obj_value, w, n, obj_by_k, status, x, c -- and the route are compared with
the recording. The other bounded tests pin no-op bounds to the sweep's bits and binding bounds to the oracle
within a tolerance; this one holds the binding cases still across a change to the kernels.

A call is (shape, variant). Shapes, 4 fleets (seeds 0 .. 3) each on the 80-layer model:

  fused_m64   M = 64, KS80       register route: every k > 1 is settled by sum lo > W
  fused_m24   M = 24, ks = [1]   register route: k1_alloc; under set_fleets_path("dp") k1_dp and its own split
  tables_m16  M = 16, [1,2,4,5]  table route: the greedy at k = 1, the tables at k > 1; under "dp" the tables alone
  tables_m2   M = 2, [1, 40]     table route
  tables_m1   M = 1, [1]         table route

Variants: "w" the D = 2 move box of bounds_cases at the shape's box k (w bounds only; on tables_m16, whose box k
is 2, fleets 0 and 1 keep the lower bounds alone so that their k = 1 stays open), "box" the binding kinds of
box_cases (box2, half, off, box1: one per fleet), "w_dp" / "box_dp" the same under the DP test path, "wcross" (a
crossing w pair, sum hi < W, sum lo > W and a free fleet), "ncross" / "nogpu" (box_cases' kinds on fleets 1 .. 3,
fleet 0 free) and "pin" (w_min = w_max = the k = 2 incumbent: R = 0 at k = 2, infeasible at every other k).
x / c are recorded for the shapes of at most 24 devices (the fixture's size); the other six outputs everywhere."""

from pathlib import Path

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver.fleets import fleet_table

from . import bounds_cases as bc
from . import box_cases as xc
from .test_gpu_bounds import IMAX, KS80, OUTS, fleet
from .test_gpu_box import BoxRun

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "bounded_bits.npz"
NF = 4
XC_MAX_M = 24  # x / c are recorded up to this fleet size
# shape: (route, M, ks, the k whose incumbent the move boxes are built around)
SHAPES = {"fused_m64": ("fused", 64, KS80, 1), "fused_m24": ("fused", 24, [1], 1),
          "tables_m16": ("tables", 16, [1, 2, 4, 5], 2), "tables_m2": ("tables", 2, [1, 40], 1),
          "tables_m1": ("tables", 1, [1], 1)}
BOX_KINDS = ("box2", "half", "off", "box1")
VARIANTS = {"fused_m64": ("w", "box"),
            "fused_m24": ("w", "box", "w_dp", "box_dp", "wcross", "ncross", "nogpu"),
            "tables_m16": ("w", "box", "w_dp", "box_dp", "wcross", "ncross", "nogpu", "pin"),
            "tables_m2": ("w", "box"), "tables_m1": ("w", "box")}
CALLS = [(s, v) for s in SHAPES for v in VARIANTS[s]]


def free_box(model, M):
    W = int(model.L)
    return [1] * M, [W] * M, [0] * M, [IMAX] * M


def boxes_of(model, shape, variant):
    """The four fleets' boxes (w_min, w_max, n_min, n_max) of a call; the n sides None for w bounds alone."""
    _, M, ks, kb = SHAPES[shape]
    W = int(model.L) // kb
    kind = variant.split("_")[0]
    if kind == "pin":  # the move box with D = 0
        return [bc.box(model, M, 2, s, 0) + (None, None) for s in range(NF)]
    if kind == "w":
        out = [bc.box(model, M, kb, s, 2) for s in range(NF)]
        # around a k > 1 incumbent sum hi < L: fleets 0 and 1 keep the lower side alone, so their k = 1 stays open
        return [(lo, [IMAX] * M if kb > 1 and s < 2 else hi, None, None) for s, (lo, hi) in enumerate(out)]
    if kind == "box":
        out = [xc.box(model, M, kb, s, BOX_KINDS[s]) for s in range(NF)]
        return [b if b is not None else xc.box(model, M, kb, s, "box2") for s, b in enumerate(out)]
    if kind == "wcross":
        lo, hi = [[1] * M for _ in range(NF)], [[IMAX] * M for _ in range(NF)]
        lo[0][M // 2], hi[0][M // 2] = 4, 3  # a crossing pair
        hi[1] = [1] * M                      # sum hi = M < W (at every k of the shapes that run this)
        lo[2] = [W] * M                      # sum lo > W
        return [(lo[f], hi[f], None, None) for f in range(NF)]
    assert kind in xc.BAD_KINDS or kind == "ncross"
    out = [free_box(model, M)]
    for s in range(1, NF):
        b = xc.box(model, M, kb, s, "cross" if kind == "ncross" else "nogpu")
        out.append(b if b is not None else free_box(model, M))
    return out


_RUNS = {}


def run_of(model, shape):
    if shape not in _RUNS:
        _, M, ks, _ = SHAPES[shape]
        _RUNS[shape] = BoxRun(fleet_table([fleet(M, s) for s in range(NF)], model), model, ks)
    return _RUNS[shape]


def replay(ctx, model, shape, variant):
    """One call: (the eight outputs, the route)."""
    route, M, ks, _ = SHAPES[shape]
    run = run_of(model, shape)
    boxes = boxes_of(model, shape, variant)
    bd.set_bounds_path(ctx, 3 if route == "tables" else 0)
    ctx.set_fleets_path("dp" if variant.endswith("_dp") else "fused")
    try:
        if boxes[0][2] is None:
            lo, hi = bc.flat([(b[0], b[1]) for b in boxes], run.table)
            return run.bounded(ctx, lo, hi)
        return run.boxed(ctx, xc.flat(boxes, run.table))
    finally:
        ctx.set_fleets_path("fused")
        bd.set_bounds_path(ctx, 0)


def recorded(shape):
    """The outputs the fixture holds for a shape."""
    return OUTS if SHAPES[shape][1] <= XC_MAX_M else tuple(f for f in OUTS if f not in ("x", "c"))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("shape,variant", CALLS, ids=[f"{s}-{v}" for s, v in CALLS])
def test_binding_bounds_keep_their_recorded_bits(llama_online_model, golden, shape, variant):
    got, route = replay(lh.get_context(0), llama_online_model, shape, variant)
    assert route == SHAPES[shape][0] == str(golden[f"{shape}/{variant}/route"])
    for f in recorded(shape):
        want = golden[f"{shape}/{variant}/{f}"]
        assert got[f].dtype == want.dtype and got[f].shape == want.shape, f
        assert np.array_equal(got[f].view(np.uint8), want.view(np.uint8)), f


def test_the_recording_holds_plans_verdicts_and_every_call(golden):
    """The fixture is not vacuous: every call is there, the binding calls hold plans and the bad ones verdicts."""
    for shape, variant in CALLS:
        st = golden[f"{shape}/{variant}/status"]
        if variant in ("w", "box", "w_dp", "box_dp", "pin"):
            assert (st == lh.STATUS_OPTIMAL).any(), (shape, variant)
        else:
            assert (st == lh.STATUS_INFEASIBLE).any() and (golden[f"{shape}/{variant}/best_k"] == 0).any()
    assert GOLDEN.stat().st_size < 100_000
