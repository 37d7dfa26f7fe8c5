"""Generate tests/golden/budget.json: the total-move-budget frontier of every case of tests/budget_cases.py.

Run:  python tests/golden/gen_budget.py      (needs the built oracle, `make -C oracle`; about a minute)

Both oracles are this repository's own code (tests/budget_cases.py): (a) the enumeration of every deviation
vector with the exact solver pinned on w, (b) HiGHS at mip_gap = 0 with the budget rows, its w re-priced by
the pinned exact solver. The file holds recorded results only:

  "A": {"M,k,s": {"w0": [...], "obj": {p: obj_value or null}, "free_p": sum max(0, w* - w0) of the exact free
        optimum w* at that k}}                                     list A, oracle (a), checked against (b)
  "B": {"M,k,s": {"w0": [...], "obj": {p: ...}, "free_p": ...}}  list B, oracle (b), checked against pinned-exact
  "edge": {name: {"obj": {p: ...}}}                              the edge shapes, by the oracle each names
  "P": {"M,scale,k,s": {"w0", "obj", "free_p", "free_unique"}}   list P (memory-pressured fleets), oracle (a) for
                                                                 M = 5 checked against (b), oracle (b) elsewhere

A disagreement between the two oracles beyond 1e-9 relative STOPS the generator.
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.append(str(REPO))


def main():
    from distilp_amd.common import ModelProfileSplit
    from distilp_amd.synth import load_model_dict
    from tests import budget_cases as bu
    from tests.bounds_cases import rel

    from oracle import milp_oracle as mo

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    out = {"A": {}, "B": {}, "edge": {}, "P": {}}

    def free_p(prob, w0):
        st, x, b1, b2, _ = mo.exact_solve(prob)
        assert st == 0 and mo.uniqueness_margin_ok(b1, b2)
        return sum(max(0, int(round(v)) - b) for v, b in zip(x[:prob["M"]], w0))

    for M, k, s in bu.LIST_A:
        devs, w0 = bu.list_case(model, M, k, s)
        prob = bu.problem(model, devs, k)
        a = bu.enumerate_frontier(prob, w0, bu.PS_A)
        for p in bu.PS_A:
            b, _ = bu.highs_budget(prob, w0, p)
            assert a[p] is not None and b is not None and rel(a[p], b) <= 1e-9, (M, k, s, p, a[p], b)
        out["A"][bu.key(M, k, s)] = {"w0": w0, "obj": {str(p): a[p] for p in bu.PS_A}, "free_p": free_p(prob, w0)}
    steps = better = 0
    for M, k, s in bu.LIST_B:
        devs, w0 = bu.list_case(model, M, k, s)
        prob = bu.problem(model, devs, k)
        pin = bu.Pinned(prob)
        objs = {}
        for p in bu.PS_B:
            b, w = bu.highs_budget(prob, w0, p)
            assert b is not None, (M, k, s, p)
            e = pin(w)
            assert e is not None and rel(b, e) <= 1e-9, (M, k, s, p, b, e)
            assert sum(w) == prob["W"] and sum(max(0, x - y) for x, y in zip(w, w0)) <= p, (M, k, s, p, w)
            objs[p] = e
        for p, q in zip(bu.PS_B, bu.PS_B[1:]):
            steps += 1
            better += objs[q] < objs[p]
        out["B"][bu.key(M, k, s)] = {"w0": w0, "obj": {str(p): objs[p] for p in bu.PS_B}, "free_p": free_p(prob, w0)}
    print(f"list B: {better} of {steps} steps between consecutive budgets strictly improve")
    steps = better = 0
    for M, sc, k, s in bu.LIST_P:
        w0, objs, fp, uniq = bu.list_p_answer(model, M, sc, k, s)
        ps = bu.ps_of_p(M)
        steps += len(ps) - 1
        better += sum(objs[q] < objs[p] for p, q in zip(ps, ps[1:]))
        out["P"][bu.key_p(M, sc, k, s)] = {"w0": w0, "obj": {str(p): objs[p] for p in ps}, "free_p": fp,
                                          "free_unique": uniq}
    print(f"list P: {better} of {steps} steps between consecutive budgets strictly improve")
    for name, e in bu.edge_cases(model).items():
        ans = bu.edge_answer(model, e)
        out["edge"][name] = {"obj": {str(p): ans[p] for p in sorted(ans)}}
        print(name, [ans[p] for p in sorted(ans)])
    (HERE / "budget.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
