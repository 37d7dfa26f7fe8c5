"""Generate tests/golden/plans.json: neighbour plans of the recorded per-k plans, priced by the project's oracle.

Run:  python tests/golden/gen_plans.py      (needs scipy's HiGHS; about a minute)

For the synthetic goldens of 2, 3, 4, 8, 16 and 64 devices (synthetic_M{M}.json, the first FLEETS[M] fleets),
every successful recorded per-k plan (k, w, n) gets six neighbours, drawn with a fixed seed: two with one
layer moved between two devices (w_i - 1, w_j + 1, n kept), two with n_i + 1, two with n_i - d, d in 1..3
(on a device with n_i > 0, d cut to n_i; a plan whose n is all zero gets another n_i + 1 instead). Each neighbour carries the answer of oracle.milp_oracle for the fixed-k MILP with the w and n
columns fixed to the plan: lower_dense, lb = max(lb, plan) and ub = min(ub, plan) on those columns (a plan
entry outside a column's own bounds is infeasible without a solve), highs_solve(mip_gap=None) -- `success`
and, when it succeeds, `objective_value` (objective_value of the returned x: c.x + sum t_comm + sum xi +
kappa). The file holds data only.

Both classes must be well represented: the generator asserts at least 25 % feasible and at least 25 %
infeasible neighbours (tests/test_plans.py asserts it on the file).
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.append(str(REPO))

SEED = 20261019
FLEETS = {2: 6, 3: 6, 4: 6, 8: 4, 16: 3, 64: 6}  # fleets taken per golden (every successful k of each)
KV = 0.5  # the synthetic goldens' kv_bits = "4bit"


def neighbours(rng, w, n):
    """Six neighbours of (w, n): (kind, w', n')."""
    M = len(w)
    out = []
    for _ in range(2):  # one layer moved i -> j
        if M < 2:
            break
        src = [i for i in range(M) if w[i] >= 2] or list(range(M))
        i = int(rng.choice(src))
        j = int(rng.choice([q for q in range(M) if q != i]))
        w2 = list(w)
        w2[i] -= 1
        w2[j] += 1
        out.append(("move", w2, list(n)))
    for _ in range(2):  # n_i + 1
        i = int(rng.integers(M))
        n2 = list(n)
        n2[i] += 1
        out.append(("n_plus", list(w), n2))
    for _ in range(2):  # n_i - d
        pos = [i for i in range(M) if n[i] > 0]
        if not pos:
            i = int(rng.integers(M))
            n2 = list(n)
            n2[i] += 1
            out.append(("n_plus", list(w), n2))
            continue
        i = int(rng.choice(pos))
        d = min(int(rng.integers(1, 4)), n[i])
        n2 = list(n)
        n2[i] -= d
        out.append(("n_minus", list(w), n2))
    return out


def price(mo, devs, model, k, w, n, sets):
    """(success, objective_value or None) of the fixed-k MILP with the w / n columns fixed."""
    p = mo.lower_dense(devs, model, k, KV, sets)
    M = p["M"]
    v = np.asarray(list(w) + list(n), float)
    lb, ub = p["lb"].copy(), p["ub"].copy()
    lb[:2 * M] = np.maximum(lb[:2 * M], v)
    ub[:2 * M] = np.minimum(ub[:2 * M], v)
    if (lb > ub).any():
        return False, None
    p["lb"], p["ub"] = lb, ub
    res = mo.highs_solve(p, mip_gap=None)
    if not res.success:
        return False, None
    return True, mo.objective_value(p, res.x)


def main():
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.synth import load_model_dict
    from oracle import milp_oracle as mo

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    rng = np.random.default_rng(SEED)
    cases = []
    for M, nfl in FLEETS.items():
        G = json.loads((HERE / f"synthetic_M{M}.json").read_text())
        for fl in G["fleets"][:nfl]:
            devs = [DeviceProfile.model_validate(d) for d in fl["devices"]]
            sets = mo.sets_of(devs)
            for rec in fl["per_k"]:
                if not rec["success"]:
                    continue
                nb = neighbours(rng, rec["w"], rec["n"])
                assert len(nb) >= 6 or M < 2
                for kind, w, n in nb:
                    ok, obj = price(mo, devs, model, rec["k"], w, n, sets)
                    cases.append({"M": M, "seed": fl["seed"], "k": rec["k"], "kind": kind, "w": w, "n": n,
                                  "success": ok, "objective_value": obj})
    feas = sum(c["success"] for c in cases)
    print(f"{len(cases)} neighbours, {feas} feasible, {len(cases) - feas} infeasible", file=sys.stderr)
    assert feas >= 0.25 * len(cases) and len(cases) - feas >= 0.25 * len(cases), "one class is under-represented"
    out = {"seed": SEED, "kv_bits": "4bit", "fleets": FLEETS, "cases": cases}
    (HERE / "plans.json").write_text(json.dumps(out, indent=None, separators=(",", ":")))


if __name__ == "__main__":
    main()
