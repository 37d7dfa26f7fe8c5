"""Generate tests/golden/change.json: the change frontier of every case of tests/change_cases.py.

Run:  python tests/golden/gen_change.py      (needs the built oracle, `make -C oracle`; a few minutes)

Both oracles are this repository's own code (tests/change_cases.py): (a) the enumeration of every deviation
vector with the exact solver pinned on w, (b) HiGHS at mip_gap = 0 with the release rows, its w re-priced by
the pinned exact solver. The file holds recorded results only. Per list, keyed "M,k,s,lost" (list P:
"M,1/scale,k,s,lost"):

  {"w0": the survivors' layers, "D": the deficit, "obj": {p: obj_value or null},
   "free_released": the layers the exact free optimum of the survivors at k takes off them (null: no plan),
   "free_unique": whether that optimum is unique}

  "A": parents of 4 and 5 devices, oracle (a) checked against (b)      "B": 8 and 16 devices, oracle (b)
  "W": the 64-device parent, oracle (b)                                "S": stale incumbents, (a) against (b)
  "P": memory-pressured parents, (a) against (b) for M = 5, (b) for M = 16
  "edge": {name: {"obj": {p: ...}}}                                    the edge shapes, by the oracle each names

A disagreement between the two oracles beyond 1e-9 relative STOPS the generator, and so does an (M, k > 1) group
(any list S group) without a step between consecutive budgets that strictly improves, or fewer than two thirds of
the lists whose free optimum lies within the largest P the launch's gate admits."""

from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.append(str(REPO))


def main():
    from distilp_amd.common import ModelProfileSplit
    from distilp_amd.solver import change as ch
    from distilp_amd.synth import load_model_dict
    from tests import change_cases as cc

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    out = {"A": {}, "B": {}, "W": {}, "S": {}, "P": {}, "edge": {}}
    reach = [0, 0]

    def record(name, k_, devs, w, ps, oracle, group, stats):
        M, k = len(devs), k_
        for lost in range(M):
            _, listed, w0 = cc.lose(devs, w, lost)
            ans = cc.answer(model, listed, k, w0, ps, oracle, tag=(name, group, lost))
            fr, uniq = cc.free_optimum(model, listed, k, w0)
            D = int(model.L) // k - sum(w0)
            yield lost, {"w0": w0, "D": D, "obj": {str(p): ans[p] for p in ps}, "free_released": fr,
                         "free_unique": uniq}
            vals = [ans[p] for p in ps]
            st = stats.setdefault(group, [0, 0])
            for a, b in zip(vals, vals[1:]):
                st[1] += 1
                st[0] += (a is None and b is not None) or (a is not None and b is not None and b < a)
            if fr is not None:
                reach[1] += 1
                reach[0] += fr <= cc.gate_p(ch, M - 1, D, k)

    stats = {}
    for name, cases, oracle in (("A", cc.LIST_A, "ab"), ("B", cc.LIST_B, "b"), ("W", [cc.WIDE], "b")):
        for M, k, s in cases:
            devs, w = cc.parent(model, M, k, s)
            for lost, rec in record(name, k, devs, w, cc.ps_of(M), oracle, (name, M, k), stats):
                out[name][cc.key(M, k, s, lost)] = rec
    for M, k, s in cc.LIST_S:
        devs, w = cc.stale_parent(model, M, k, s)
        for lost, rec in record("S", k, devs, w, cc.PS_A, "ab", ("S", M, k), stats):
            out["S"][cc.key(M, k, s, lost)] = rec
    for M, sc, k, s in cc.LIST_P:
        devs, w = cc.parent(model, M, k, s, sc)
        for lost, rec in record("P", k, devs, w, cc.ps_of(M), "ab" if M <= 5 else "b", ("P", M, k), stats):
            out["P"][cc.key_p(M, sc, k, s, lost)] = rec
    for g, (better, steps) in sorted(stats.items()):
        print(f"{g}: {better} of {steps} steps between consecutive budgets strictly improve")
        assert better >= 1 or (g[0] != "S" and g[2] == 1), g  # k = 1 around an optimal incumbent is flat
    print(f"far end: {reach[0]} of {reach[1]} lists have their free optimum within the gate")
    assert 3 * reach[0] >= 2 * reach[1]
    for name, e in cc.edge_cases(model).items():
        ans = cc.edge_answer(model, e)
        out["edge"][name] = {"obj": {str(p): ans[p] for p in sorted(ans)}}
        print(name, [ans[p] for p in sorted(ans)])
    (HERE / "change.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
