"""tests/golden/pressure_scale.json without a GPU: two parents recomputed from scratch by the oracles, the conditions
(a) .. (d) and the winner-checked share from the file alone, the parents' shapes against the launch gate, and the
scale-in entry's host logic (the enumeration hook) fed with the recorded candidate frontiers."""

import math

import pytest

from distilp_amd.solver import scale as sc

from . import pressure_cases as pc
from . import pressure_scale_cases as px
from .test_scale import point

# the capped parent (the only one with candidates that have no plan) and an irregular one with two heads
RECOMPUTED = [px.CAPPED[0], next(s for s in px.irregular() if "two_heads" in s[1][4] and s[2] == 2)]


def test_the_file_holds_every_parent_and_nothing_else():
    gold = px.golden()
    assert sorted(gold) == ["in", "out"] and list(gold["in"]) == [px.key(s) for s in px.parents()]
    edits = {e for s in px.irregular() for e in s[1][4]}
    assert set(px.IRREGULAR_EDITS) <= edits
    for spec in px.parents():
        par, rec = px.parent(spec), gold["in"][px.key(spec)]
        M = len(par["devs"])
        assert (rec["k"], rec["w0"], rec["droppable"], rec["heads"], rec["w_max"]) == (
            par["k"], par["w0"], par["droppable"], par["heads"], par["w_max"]), spec
        assert len(par["droppable"]) <= px.MAX_DROPPABLE and set(par["heads"]) <= set(par["droppable"]), spec
        assert sum(par["w0"]) == pc.L // par["k"] and min(par["w0"]) >= 1, spec
        sc.check_scale_gate([M], [par["droppable"]], [par["w0"]], pc.L // par["k"], par["k"], 0, max(px.DROPS),
                            max(par["ps"]))
        for d in px.DROPS:
            assert rec["rows"][str(d)]["gone"] == [g for g, _ in px.candidates(par, d)], (spec, d)
            assert len(rec["rows"][str(d)]["gone"]) <= 15, (spec, d)
    par = px.out_parent()
    assert gold["out"]["w0"] == par["w0"] and sorted(gold["out"]["rows"]) == ["1", "2", "3"]


@pytest.mark.parametrize("spec", RECOMPUTED, ids=px.key)
def test_a_parent_recomputed_from_scratch_equals_the_file(spec):
    rec = px.golden()["in"][px.key(spec)]
    got = px.answer(pc.our_model(), px.parent(spec), tag=px.key(spec))
    assert got["rows"].keys() == rec["rows"].keys()
    for d, row in got["rows"].items():
        want = rec["rows"][d]
        assert row["gone"] == want["gone"], (spec, d)
        for c, (a, b) in enumerate(zip(row["obj"], want["obj"])):
            for p in a:
                assert (a[p] is None) == (b[p] is None), (spec, d, c, p)
                assert a[p] is None or pc.close(a[p], b[p]), (spec, d, c, p, a[p], b[p])
        for p, cell in row["cells"].items():
            w = want["cells"][p]
            assert (cell["at"], cell["slack_or_t"]) == (w["at"], w["slack_or_t"]), (spec, d, p)
            assert (cell["margin"] is None) == (w["margin"] is None), (spec, d, p)
            assert cell["margin"] is None or abs(cell["margin"] - w["margin"]) <= 1e-9, (spec, d, p)


def test_conditions_and_the_winner_checked_share_from_the_file_alone():
    gold = px.golden()
    n = px.assert_conditions(px.records(gold))
    assert n["a"] >= 1 and n["b"] >= 1 and n["c"] >= 1 and n["d"] >= 1
    assert n["checked"] >= 0.9 * n["feasible"] > 0
    # a cell's recorded minimum is its candidates' strict earliest minimum
    for name, rec in px.records(gold).items():
        for d, row in rec["rows"].items():
            for p, cell in row["cells"].items():
                at, least = px.sx.best([o[p] for o in row["obj"]])
                assert (cell["at"], cell["obj"]) == (at, least), (name, d, p)
                assert at is None or cell["margin"] == px.margin([o[p] for o in row["obj"]], at), (name, d, p)


@pytest.mark.parametrize("spec", px.parents(), ids=px.key)
def test_hook_fed_with_the_recorded_frontiers_returns_the_recorded_winners(spec):
    """halda_scale_in_frontier's host logic on the recorded candidate frontiers: per cell the recorded minimum, and
    the recorded winner where the cell strictly improves on the cell before it (else the running minimum may keep
    the earlier list)."""
    rec, par = px.golden()["in"][px.key(spec)], px.parent(spec)
    M, ps = len(par["devs"]), par["ps"]
    by = {tuple(g): o for row in rec["rows"].values() for g, o in zip(row["gone"], row["obj"])}

    def solve(lists):
        out = []
        for kept in lists:
            o = by[tuple(i for i in range(M) if i not in kept)]
            out.append([point(p, o[str(p)]) for p in ps])
        return out

    rows = sc.halda_scale_in_frontier(par["devs"], pc.our_model(), (par["k"], par["w0"], [0] * M), max(px.DROPS),
                                      max(ps), keep=par["keep"], _solve_lists=solve)
    for d, row in zip(px.DROPS, rows):
        last = math.inf
        for p, pt in enumerate(row):
            cell = rec["rows"][str(d)]["cells"][str(p)]
            if cell["obj"] is None:
                assert pt.point.plan is None and pt.dropped == [] and pt.kept == [], (spec, d, p)
                continue
            assert pt.point.obj_value == cell["obj"] <= last, (spec, d, p)
            if cell["obj"] < last:
                assert pt.dropped == rec["rows"][str(d)]["gone"][cell["at"]], (spec, d, p)
            last = cell["obj"]
