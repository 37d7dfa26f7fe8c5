"""Generate tests/golden/scale.json: the answers of tests/scale_cases.py.

Run:  python tests/golden/gen_scale.py      (needs the built oracle, `make -C oracle`, and tests/golden/change.json)

Recorded results only, by this repository's own oracles (tests/change_cases.py): (a) the enumeration of every
deviation vector with the exact solver pinned on w, checked against (b) HiGHS at mip_gap = 0 with the release rows.

  "pairs": {"M,k,s,i-j": {"w0": the survivors' layers, "D": the deficit, "obj": {p: obj_value or null}}}
           every pair (i, j) lost from every parent of scale_cases.PARENTS (change_cases.LIST_S) and EXTRA
  "cells": {"M,k,s": {p: {"obj": the least pair objective or null, "pair": [i, j] of the strict earliest minimum,
                          "greedy": the pair a greedy repeat of the best single loss picks}}}
  "out":   {"none" | "j" | "i+j": {"w0": ..., "obj": {p: ...}}}   the scale-out case, by oracle (a)

The generator STOPS when the two oracles disagree beyond 1e-9 relative, or when an (M, k) group has no d = 2 cell
whose winner is strictly better than the greedy pair (scale_cases.NO_GAP names the group where the searched seeds
have none): without such a cell the tests could not tell the exact pick from a greedy one."""

from __future__ import annotations

import itertools
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.append(str(REPO))


def main():
    from distilp_amd.common import ModelProfileSplit
    from distilp_amd.synth import load_model_dict
    from tests import change_cases as cc
    from tests import scale_cases as sc

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    single = cc.golden()["S"]
    out = {"pairs": {}, "cells": {}, "out": {}}
    differs = {}
    for M, k, s in sc.PARENTS + sc.EXTRA:
        devs, w = cc.stale_parent(model, M, k, s)
        objs = {}
        for pair in sc.pairs(M):
            _, listed, w0 = cc.lose(devs, w, pair)
            ans = cc.answer(model, listed, k, w0, sc.PS, "ab", tag=(M, k, s, pair))
            objs[pair] = ans
            out["pairs"][sc.pair_key(M, k, s, pair)] = {"w0": w0, "D": int(model.L) // k - sum(w0),
                                                        "obj": {str(p): ans[p] for p in sc.PS}}
            print(sc.pair_key(M, k, s, pair), [ans[p] for p in sc.PS], flush=True)
        if (M, k, s) in sc.PARENTS:  # the single losses are change.json's list S
            one = [{p: single[cc.key(M, k, s, i)]["obj"][str(p)] for p in sc.PS} for i in range(M)]
        else:
            one = [cc.answer(model, cc.lose(devs, w, i)[1], k, cc.lose(devs, w, i)[2], sc.PS, "a") for i in range(M)]
        cells = {}
        for p in sc.PS:
            ps = sc.pairs(M)
            at, least = sc.best([objs[q][p] for q in ps])
            g = sc.greedy_pair(one, objs, M, p)
            cells[str(p)] = {"obj": least, "pair": None if at is None else list(ps[at]),
                             "greedy": None if g is None else list(g)}
            if at is not None and g is not None and objs[g][p] is not None and least < objs[g][p]:
                differs[(M, k)] = differs.get((M, k), 0) + 1
        out["cells"][f"{M},{k},{s}"] = cells
    for g in sorted({(M, k) for M, k, _ in sc.PARENTS}):
        print(f"{g}: {differs.get(g, 0)} d = 2 cells whose winner beats the greedy pair")
        assert (differs.get(g, 0) >= 1) != (g in sc.NO_GAP), g
    devs, w, pool = sc.out_case(model)
    k = sc.OUT[1]
    for a in range(sc.OUT_ADD + 1):
        for added in itertools.combinations(range(len(pool)), a):
            listed, w0 = devs + [pool[j] for j in added], list(w) + [0] * a
            ans = cc.answer(model, listed, k, w0, sc.PS, "a", tag=("out", added))
            out["out"][sc.out_key(added)] = {"w0": w0, "obj": {str(p): ans[p] for p in sc.PS}}
            print("out", added, [ans[p] for p in sc.PS], flush=True)
    (HERE / "scale.json").write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {HERE / 'scale.json'}")


if __name__ == "__main__":
    main()
