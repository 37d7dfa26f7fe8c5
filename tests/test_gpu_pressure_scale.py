"""Scale-in / scale-out on the GPU (halda_solve_change_subsets: index kernel, change kernel, pick kernel) on the
memory-pressured and irregular parents of tests/pressure_scale_cases.py, against tests/golden/pressure_scale.json:
the change oracle's answer of EVERY candidate list, not another GPU route. Feasibility per cell exactly, obj_value
within 1e-9 relative, the candidate returned is one whose recorded objective reaches the minimum and, where the
margin to the best other candidate exceeds 1e-9, THE recorded winner; the identities of test_gpu_scale.py with the
failover and change entries; and a chunked raw grid, an infeasible candidate and the winner in different launches."""

import math

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import change as ch
from distilp_amd.solver import scale as sc
from distilp_amd.solver.fleets import fleet_table

from . import pressure_cases as pc
from . import pressure_scale_cases as px
from .test_gpu_scale import FIELDS, check_row, same

pytestmark = pytest.mark.gpu

KVB = "4bit"
_TALLY = dict(cells=0, feasible=0, checked=0)


def check_cell(pt, rec, d, p, M, tag):
    """One cell against the record of its row; whether the winner was checked."""
    row = rec["rows"][str(d)]
    cell = row["cells"][str(p)]
    assert (pt.point.plan is None) == (cell["obj"] is None), (tag, pt.point.obj_value, cell)
    _TALLY["cells"] += 1
    if cell["obj"] is None:
        assert pt.dropped == [] and pt.kept == [] and pt.point == ch.ChangePoint(p, None, math.inf, 0, 0, math.inf), tag
        return False
    _TALLY["feasible"] += 1
    assert pc.close(pt.point.obj_value, cell["obj"]), (tag, pt.point.obj_value, cell)
    assert sorted(pt.dropped + pt.kept) == list(range(M)) and len(pt.dropped) == d, (tag, pt.dropped, pt.kept)
    assert pt.dropped in row["gone"], (tag, pt.dropped)
    mine = row["obj"][row["gone"].index(pt.dropped)][str(p)]
    assert mine is not None and pc.close(mine, cell["obj"]), (tag, pt.dropped, mine, cell)
    if cell["margin"] is None or cell["margin"] > px.MARGIN:
        assert pt.dropped == row["gone"][cell["at"]], (tag, pt.dropped, row["gone"][cell["at"]], cell)
        _TALLY["checked"] += 1
        return True
    return False


@pytest.mark.parametrize("spec", px.parents(), ids=px.key)
def test_scale_in_equals_the_change_oracle(spec):
    model, rec, par = pc.our_model(), px.golden()["in"][px.key(spec)], px.parent(spec)
    devs, k, w, ps = par["devs"], par["k"], par["w0"], par["ps"]
    M, P = len(devs), max(par["ps"])
    assert rec["w0"] == w and rec["droppable"] == par["droppable"] and ps == tuple(range(P + 1))
    inc, cap = (k, w, [0] * M), par["w_max"]
    assert rec["w_max"] == cap
    fr = sc.halda_scale_in_frontier(devs, model, inc, max(px.DROPS), P, keep=par["keep"], kv_bits=KVB, w_max=cap)
    assert len(fr) == len(px.DROPS) and all(len(r) == P + 1 for r in fr)
    for d, row in zip(px.DROPS, fr):
        for p, pt in enumerate(row):
            check_cell(pt, rec, d, p, M, (px.key(spec), d, p))
        check_row(row, pc.L // k, w, (px.key(spec), d))
        for pt in row:
            assert not set(pt.dropped) & set(par["keep"]), (spec, d, pt.dropped)
        lost = {tuple(pt.dropped) for pt in row if pt.point.plan is not None and pt.dropped}
        by = {g: ch.halda_failover_frontiers(devs, model, inc, P, [g], KVB, w_max=cap)[0] for g in lost}
        for p, pt in enumerate(row):
            if pt.point.plan is not None and d:
                assert pt.point == by[tuple(pt.dropped)][p], (spec, d, p)
    assert [pt.point for pt in fr[0]] == ch.halda_change_frontier(devs, model, k, w, P, KVB, w_max=cap)
    print(f"{px.key(spec)}: {sum(len(r['gone']) for r in rec['rows'].values())} candidates, tally {_TALLY}")


def test_scale_out_equals_the_change_oracle():
    model, rec, par = pc.our_model(), px.golden()["out"], px.out_parent()
    M, q, k, w, P = par["n_fleet"], px.OUT_POOL, par["k"], par["w0"], max(par["ps"])
    devs, pool = par["devs"][:M], par["pool"]
    assert rec["w0"] == w
    fr = sc.halda_scale_out_frontier(devs, pool, model, (k, w[:M], [0] * M), px.OUT_ADD, P, KVB)
    assert len(fr) == px.OUT_ADD + 1
    for a, row in enumerate(fr):
        for p, pt in enumerate(row):
            if check_cell(pt, rec, q - a, p, M + q, ("out", a, p)) or pt.point.plan is not None:
                assert pt.added == [i - M for i in pt.kept if i >= M] and len(pt.added) == a, ("out", a, p)
                assert pt.kept[:M] == list(range(M)), ("out", a, p)
        check_row(row, pc.L // k, w, ("out", a))
    assert [pt.point for pt in fr[0]] == ch.halda_change_frontier(devs, model, k, w[:M], P, KVB)
    assert any(pt.point.plan is None for pt in fr[1]) and any(pt.point.plan is not None for pt in fr[2])


def test_most_feasible_cells_have_one_recorded_winner():
    """A condition on the case list (gen_pressure_scale.py asserts it on the oracle's answers): at least 90 % of the
    feasible cells are winner-checked, and the conditions (a) .. (d) hold."""
    n = px.assert_conditions(px.records(px.golden()))
    print(f"{n['cells']} cells, {n['feasible']} feasible, {n['checked']} winner-checked; (a) {n['a']} (b) {n['b']} "
          f"(c) {n['c']} (d) {n['d']}; no (a) cell in {sorted(px.NO_CASE['a'])}")


def test_chunked_grid_with_a_planless_candidate_before_the_winner_is_byte_identical():
    """The raw grid of the pressured parent with cells of condition (a) -- a candidate without a plan before the
    winner --, one chunk against a cap of ONE candidate of the longest list: the two fall into different launches."""
    model, gold = pc.our_model(), px.golden()["in"]
    name, d, p = next(c for c in px.conditions(gold)["a_keys"] if c[1] >= 1)
    spec = next(s for s in px.PRESSURED + px.CAPPED if px.key(s) == name)
    par = px.parent(spec)
    devs, k, P = par["devs"], par["k"], max(par["ps"])
    M = len(devs)
    table = fleet_table([devs], model)
    w0 = np.asarray(par["w0"], np.int32)
    masks = np.asarray([sc._mask(par["keep"])], np.uint64)
    dmax = max(px.DROPS)
    cap = None if par["w_max"] is None else np.asarray(par["w_max"], np.int32)

    def run():
        return sc.solve_change_subsets_table(table, model, k, w0, 0, dmax, P, pc.kv_factor(KVB), masks, None, cap)

    one = run()
    ctx = lh.get_context(0)
    sc.set_change_subsets_chunk(ctx, sc.launch_bytes(M, P, 1))
    try:
        many = run()
    finally:
        sc.set_change_subsets_chunk(ctx, 0)
    same(many, one, name)
    assert set(FIELDS) == {"status", "obj", "dropped_mask", "loaded", "released", "w", "n"}
    # the grid itself against the record: the cell of condition (a) has a plan, and its mask is the recorded winner's
    rec = gold[name]
    for dd in px.DROPS:
        row = rec["rows"][str(dd)]
        for pp in par["ps"]:
            cell = row["cells"][str(pp)]
            assert (one.status[0, dd, pp] == lh.STATUS_OPTIMAL) == (cell["obj"] is not None), (name, dd, pp)
            if cell["obj"] is None:
                assert np.isinf(one.obj[0, dd, pp]) and not one.w[0, dd, pp].any(), (name, dd, pp)
            elif cell["margin"] is None or cell["margin"] > px.MARGIN:
                assert int(one.dropped_mask[0, dd, pp]) == sc._mask(row["gone"][cell["at"]]), (name, dd, pp)
    row = rec["rows"][str(d)]
    at = row["cells"][str(p)]["at"]
    assert at >= 1 and any(o[str(p)] is None for o in row["obj"][:at])
    print(f"{name}: cell d = {d}, p = {p}: winner is candidate {at} of {len(row['gone'])}, "
          f"{sum(o[str(p)] is None for o in row['obj'][:at])} planless candidates before it")
