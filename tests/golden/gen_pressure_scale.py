"""Generate tests/golden/pressure_scale.json: the answers of tests/pressure_scale_cases.py.

Run:  python tests/golden/gen_pressure_scale.py      (needs the built oracle, `make -C oracle`)

Recorded results and index lists only, by this repository's own oracles (tests/change_cases.py): per candidate list
the enumeration of every deviation vector with the exact solver pinned on w, asserted equal to HiGHS at mip_gap = 0
with the release rows (lists of at most five survivors), or HiGHS re-priced by the pinned exact solver (wider lists).

  "in":  {parent key: {"k", "w0", "droppable", "heads",
                       "rows": {d: {"gone": the dropped index list of every candidate, in candidate order,
                                    "obj":  per candidate {p: obj_value or null},
                                    "cells": {p: {"obj": the least objective or null, "at": the earliest candidate
                                                  that reaches it, "margin": the relative distance to the best OTHER
                                                  candidate (null: none has a plan), "slack_or_t": whether the
                                                  winning plan has a positive slack or t column}}}}}}
  "out": the scale-out case, one such record over devs + pool (row d adds OUT_POOL - d pool devices)

The generator STOPS when the two oracles disagree beyond 1e-9 relative, when one of the conditions (a) .. (d) of
pressure_scale_cases.conditions has no cell (pressure_scale_cases.NO_CASE names a class where a 40-seed search finds
none), when fewer than 90 % of the feasible cells have one winner (margin above 1e-9), or when no reload ladder of
tests/pressure_reload_cases.py has two consecutive optima that differ in a slack or t column."""

from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.append(str(REPO))


def main():
    from tests import pressure_cases as pc
    from tests import pressure_reload_cases as rc
    from tests import pressure_scale_cases as px

    model = pc.our_model()
    say = lambda s: print(s, flush=True)  # noqa: E731
    out = {"in": {}, "out": None}
    for spec in px.parents():
        name = px.key(spec)
        out["in"][name] = px.answer(model, px.parent(spec), tag=name, log=say)
    out["out"] = px.answer(model, px.out_parent(), drops=range(px.OUT_POOL - px.OUT_ADD, px.OUT_POOL + 1), tag="out",
                           log=say)
    n = px.assert_conditions(px.records(out))
    print(f"{len(out['in'])} scale-in parents and the scale-out case, {n['cells']} cells, {n['feasible']} feasible, "
          f"{n['checked']} winner-checked ({n['checked'] / n['feasible']:.1%})")
    print(f"(a) {n['a']} cells with a planless candidate before the winner; (b) {n['b']} (parent, d) with no plan at a "
          f"small p and one at a larger p; (c) {n['c']} irregular cells whose winner drops a head; (d) {n['d']} cells "
          f"whose winning plan uses a slack or t")
    steps = {f: rc.slack_steps(f) for f in rc.FLEETS}
    print(f"condition (a) cells: {n['a_keys']}; NO_CASE: {px.NO_CASE}")
    print("reload ladders, the j whose optimum differs from point j + 1's in a slack or t column:", steps)
    assert any(steps.values()), steps
    (HERE / "pressure_scale.json").write_text(json.dumps(out, indent=None, separators=(",", ":")) + "\n")
    print(f"wrote {HERE / 'pressure_scale.json'}")


if __name__ == "__main__":
    main()
