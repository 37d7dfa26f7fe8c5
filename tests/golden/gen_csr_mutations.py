"""Generate tests/golden/csr_mutations.json: HiGHS's answers to tests/csr_mutation_cases.py.

Run:  python tests/golden/gen_csr_mutations.py      (needs scipy and the built oracle, `make -C oracle`)

Recorded results only, by scipy.optimize.milp (HiGHS) at mip_gap = 0 on the mutated dense problem
(oracle.milp_oracle.highs_solve):

  "bases": {name: {"fun": the unmutated optimum c.x,
                   "cases": [{"kind", "cls": "K" | "R" | "E", "dev": the device the kind was applied to,
                              "success", "fun": c.x or null, "changed": fun differs from the base's by more
                              than 1e-6 relative (or the verdict does)}
                             | {..., "highs": "error"} where scipy refuses the problem (an infinite rhs)]}}

No x is stored. For a K kind the devices are tried in order and the first whose mutation changes the optimum is
kept (the first the kind applies to when none does); the search itself uses the exact oracle, the recorded
answer is HiGHS's. R and E kinds take the first device they apply to. The generator STOPS unless at least half
of the K cases changed the optimum: a K case that leaves it alone cannot tell a decoder that honours the
mutation from one that drops it."""

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
    from oracle import milp_oracle as mo
    from tests import csr_mutation_cases as mc

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()

    def differs(fun, base):
        return fun is None or abs(fun - base) > 1e-6 * max(1.0, abs(base))

    out = {"bases": {}}
    n_k = n_changed = 0
    for base in mc.BASES:
        P = mc.base_dense(model, base)
        S = mc.Shape(P)
        res0 = mo.highs_solve(mc.to_prob(P), mip_gap=0.0)
        assert res0.success, base
        fun0 = float(res0.fun)
        recs = []
        for kind in mc.kinds_of(base[3]):
            cls = mc.KINDS[kind]
            dev = mc.first_device(kind, S)
            if dev is None:
                print(base[0], kind, "applies to no device", flush=True)
                continue
            if cls == "K":  # the first device whose mutation moves the optimum
                for i in range(S.M):
                    ops = mc.make(kind, S, i)
                    if ops is None:
                        continue
                    st, _, b1, _, _ = mo.exact_solve(mc.to_prob(mc.apply(P, ops)))
                    assert st in (0, 2), (base, kind, i, st)
                    if differs(b1 if st == 0 else None, fun0):
                        dev = i
                        break
            Q = mc.to_prob(mc.apply(P, mc.make(kind, S, dev)))
            rec = {"kind": kind, "cls": cls, "dev": dev}
            try:
                res = mo.highs_solve(Q, mip_gap=0.0)
            except ValueError as e:
                assert cls == "R", (base, kind, e)
                rec["highs"] = "error"
                recs.append(rec)
                continue
            fun = float(res.fun) if res.success else None
            rec.update(success=bool(res.success), fun=fun, changed=bool(differs(fun, fun0)))
            if cls == "K":
                n_k += 1
                n_changed += rec["changed"]
            recs.append(rec)
            print(base[0], rec, flush=True)
        out["bases"][base[0]] = {"fun": fun0, "cases": recs}
    print(f"K cases: {n_k}, of which {n_changed} change the optimum")
    assert 2 * n_changed >= n_k, (n_changed, n_k)
    (HERE / "csr_mutations.json").write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {HERE / 'csr_mutations.json'}")


if __name__ == "__main__":
    main()
