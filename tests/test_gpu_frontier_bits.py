"""The move and change frontier kernels (halda_sweep_budget_kernel, halda_sweep_change_kernel) and the scale
entry that runs the second, pinned bit for bit (tests/golden/frontier_bits.npz, recorded by
tests/golden/gen_frontier_bits.py from the build BEFORE the two kernels were given one body): every call of CALLS
is replayed through solve_budget_table / solve_change_table / solve_change_subsets_table and every output array
is compared with the recording -- status, obj as uint64, moved or loaded / released, w and n (the scale grid's
dropped_mask too). The other frontier tests hold the kernels to the oracle within a tolerance and to each other;
this one holds their bytes still across a change to the shared body.

The calls are existing case definitions, each a few devices:

  budget/A3/k*      budget_cases.LIST_A's 3-device fleets alone: the uniform-extent launch (k = 1, 2), P = 3
  budget/A34/k*     its 3- and 4-device fleets in one launch: mixed extents (k = 1, 2; k = 4 has M = 4 alone)
  budget/<edge>     one_device, wide_64 (all 64 lanes, P = 2), cap_excludes_w0 (leading points with no plan),
                    crossing_box (settled before any table), clipped_window (k = 4), tied_k2 (the strict "<"
                    tie rules), pressured_w_min
  change/A/k*       change_cases.LIST_A, every device lost in turn: lists of 3 and 4 in one call per k, D > 0
  change/W          WIDE with devices 0, 21, 42 and 63 lost: lists of 63 at P = 2
  change/P          one LIST_P parent (5 pressured devices, k = 2), every device lost in turn
  change/<edge>     every change_cases.edge_cases entry: the joiners (a w0 = 0 entry; point 0 has no plan), the
                    w_min / w_max boxes, the clipped window, the ties
  change/D0/k2      budget_cases.LIST_A at k = 2 as identity items with max_deficit = 0
  scale/M4_k1       scale_cases' smallest parent (4 devices, k = 1, a stale incumbent), d = 0 .. 2, P = 3"""

from pathlib import Path

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import budget as bg
from distilp_amd.solver import change as ch
from distilp_amd.solver import scale as sc
from distilp_amd.solver.fleets import fleet_table
from distilp_amd.solver.subfleets import pack_items

from . import bounds_cases as bc
from . import budget_cases as bu
from . import change_cases as cc
from . import scale_cases as sx

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "frontier_bits.npz"
BUDGET_FIELDS = ("status", "obj", "moved", "w", "n")
CHANGE_FIELDS = ("status", "obj", "loaded", "released", "w", "n")
SCALE_FIELDS = ("status", "obj", "dropped_mask", "loaded", "released", "w", "n")
BUDGET_EDGES = ("one_device", "wide_64", "cap_excludes_w0", "crossing_box", "clipped_window", "tied_k2",
                "pressured_w_min")
CHANGE_EDGES = ("largest_deficit", "lost_head", "one_survivor", "two_lost", "joiner_no_deficit", "joiner_and_loss",
                "w_max_blocks_small_p", "crossing_box", "clipped_window", "tied_k2")
WIDE_LOST = (0, 21, 42, 63)


def budget_call(model, fleets, k, w0s, P, lo=None, hi=None):
    table = fleet_table(fleets, model)
    w0 = np.concatenate([np.asarray(w, np.int32) for w in w0s])
    res = bg.solve_budget_table(table, model, k, w0, P, bc.KV, None if lo is None else bg._flat(table, [lo], 0),
                                None if hi is None else bg._flat(table, [hi], bg.INT32_MAX))
    return {f: getattr(res, f) for f in BUDGET_FIELDS}


def budget_list(model, sizes, k):
    gold = bu.golden()["A"]
    sub = [c for c in bu.LIST_A if c[0] in sizes and c[1] == k]
    return [list(bc.devices(M, s)) for M, _, s in sub], [gold[bu.key(*c)]["w0"] for c in sub]


def change_call(model, parents, items, k, w0s, P, lo=None, hi=None, max_deficit=None):
    table = fleet_table(parents, model)
    packed = pack_items(table.sizes(), items)
    lens = np.diff(packed[1])
    w0 = np.concatenate([np.asarray(w, np.int32) for w in w0s])
    res = ch.solve_change_table(table, model, k, packed, w0, P, bc.KV,
                                None if lo is None else ch._flat_lists(([lo], lens), 0),
                                None if hi is None else ch._flat_lists(([hi], lens), ch.INT32_MAX), max_deficit)
    return {f: getattr(res, f) for f in CHANGE_FIELDS}


def lost_in_turn(name, parents, losses=None):
    """(parent fleets, items, w0s) of list `name`'s parents [(golden key prefix, devices)], every device (or
    each of `losses`) lost in turn; the survivors' layers are the golden file's."""
    gold = cc.golden()[name]
    fleets, items, w0s = [], [], []
    for f, (key, devs) in enumerate(parents):
        fleets.append(devs)
        for lost in range(len(devs)) if losses is None else losses:
            items.append((f, [i for i in range(len(devs)) if i != lost]))
            w0s.append(gold[f"{key},{lost}"]["w0"])
    return fleets, items, w0s


def _budget_a(sizes, k):
    def run(model):
        fleets, w0s = budget_list(model, sizes, k)
        return budget_call(model, fleets, k, w0s, max(bu.PS_A))
    return run


def _budget_edge(name):
    def run(model):
        e = bu.edge_cases(model)[name]
        return budget_call(model, [e["devs"]], e["k"], [e["w0"]], e["P"], e["w_min"], e["w_max"])
    return run


def _change_a(k):
    def run(model):
        parents = [(f"{M},{k},{s}", list(bc.devices(M, s))) for M, kk, s in cc.LIST_A if kk == k]
        fleets, items, w0s = lost_in_turn("A", parents)
        return change_call(model, fleets, items, k, w0s, max(cc.PS_A))
    return run


def _change_wide(model):
    M, k, s = cc.WIDE
    fleets, items, w0s = lost_in_turn("W", [(f"{M},{k},{s}", list(bc.devices(M, s)))], WIDE_LOST)
    return change_call(model, fleets, items, k, w0s, max(cc.PS_W))


def _change_p(model):
    from . import pressure_cases as pc

    M, scale, k, s = cc.LIST_P[0]
    fleets, items, w0s = lost_in_turn("P", [(f"{M},1/{scale.denominator},{k},{s}", pc.devices(s, M, scale))])
    return change_call(model, fleets, items, k, w0s, max(cc.ps_of(M)))


def _change_edge(name):
    def run(model):
        e = cc.edge_cases(model)[name]
        return change_call(model, [e["devs"]], [(0, e["idx"])], e["k"], [e["w0"]], e["P"], e["w_min"], e["w_max"])
    return run


def _change_d0(model):
    fleets, w0s = budget_list(model, (3, 4), 2)
    items = [(f, list(range(len(d)))) for f, d in enumerate(fleets)]
    return change_call(model, fleets, items, 2, w0s, max(bu.PS_A), max_deficit=0)


def _scale(model):
    M, k, s = min(sx.PARENTS)
    devs, w0 = cc.stale_parent(model, M, k, s)
    res = sc.solve_change_subsets_table(fleet_table([devs], model), model, k, np.asarray(w0, np.int32), 0, 2, sx.P,
                                        bc.KV, None)
    return {f: getattr(res, f) for f in SCALE_FIELDS}


CALLS = {f"budget/A3/k{k}": _budget_a((3,), k) for k in (1, 2)}
CALLS.update({f"budget/A34/k{k}": _budget_a((3, 4), k) for k in (1, 2, 4)})
CALLS.update({f"budget/{n}": _budget_edge(n) for n in BUDGET_EDGES})
CALLS.update({f"change/A/k{k}": _change_a(k) for k in (1, 2, 4)})
CALLS.update({"change/W": _change_wide, "change/P": _change_p})
CALLS.update({f"change/{n}": _change_edge(n) for n in CHANGE_EDGES})
CALLS.update({"change/D0/k2": _change_d0, "scale/M4_k1": _scale})


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("call", list(CALLS))
def test_frontier_calls_keep_their_recorded_bits(llama_online_model, golden, call):
    got = CALLS[call](llama_online_model)
    assert sorted(got) == sorted(k.rsplit("/", 1)[1] for k in golden if k.rsplit("/", 1)[0] == call)
    for f, a in got.items():
        want = golden[f"{call}/{f}"]
        assert a.dtype == want.dtype and a.shape == want.shape, (call, f)
        if a.dtype == np.float64:
            a, want = a.view(np.uint64), want.view(np.uint64)
        assert np.array_equal(a, want), (call, f)


def test_the_recording_holds_both_verdicts_and_a_scan_won_by_two_thresholds(golden):
    """The fixture is not vacuous: every call is there, the set holds OPTIMAL and INFEASIBLE points, and at
    least one k > 1 item whose points were won by more than one threshold T (the generator's count)."""
    for call in CALLS:
        assert f"{call}/status" in golden, call
    st = np.concatenate([golden[f"{c}/status"].ravel() for c in CALLS])
    assert (st == lh.STATUS_OPTIMAL).any() and (st == lh.STATUS_INFEASIBLE).any()
    assert int(golden["meta/items_won_by_several_T"]) >= 1
    assert GOLDEN.stat().st_size < 100_000
