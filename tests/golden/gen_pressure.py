"""Generate tests/golden/pressure.json from the REFERENCE implementation (this container only).

Run:  python tests/golden/gen_pressure.py      (needs /root/reference; a few seconds)

The reference is imported exactly as gen_golden.py imports it (its import_reference / run_solve). For seeds
0..3 of every (M, scale) class of tests/pressure_cases.py (0..1 of the classes of 2, 3 and 5 devices: its
golden_seeds) -- pressured_fleet(seed, M, scale): synth_fleet with
the three memory fields scaled down -- on the llama_3_70b/online model the file holds the reference's
`halda_solve` (kv 4bit, mip_gap 1e-4, its own k list) as recorded results only: the HALDAResult fields and, per
k, success / w / n / obj_value. The device dicts are not stored (pressured_fleet regenerates them).

Every recorded fleet is checked here against the exact oracle under the suite's standing rule (same status per
k; the result's objective within 1e-9 relative and its (k, w, n, sets) identical where the exact margin exceeds
1e-7; a losing k's objective within 1.5e-6, tests/test_variants.py). A disagreement STOPS the generator, as in
gen_golden_subfleets.py. The generator also asserts the "pressured" floors of tests/pressure_cases.py (FLOORS)
on the instances it writes.
"""

from __future__ import annotations

import json
import sys
from fractions import Fraction
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path.append(str(REPO))

KV, GAP = "4bit", 1e-4


def main():
    from gen_golden import import_reference, run_solve

    hp, _, DeviceProfile, ModelProfileSplit = import_reference()
    from distilp_amd.synth import load_model_dict
    from tests import pressure_cases as pc

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    fleets, inst = [], []
    for (M, scale) in pc.CLASSES:
        for seed in pc.golden_seeds(M):
            devs = [DeviceProfile.model_validate(d) for d in pc.pressured_fleet(seed, M, scale)]
            res, err, calls, _ = run_solve(hp, devs, model, KV, GAP)
            rec = {"M": M, "scale": [scale.numerator, scale.denominator], "seed": seed, "result": res, "error": err,
                   "per_k": [{k: c[k] for k in ("k", "success", "w", "n", "obj_value") if k in c} for c in calls]}
            why = pc.golden_mismatch(rec, "exact")
            if why:
                raise SystemExit(f"M={M} scale={scale} seed={seed}: the exact oracle and the reference disagree "
                                 f"({why}); see this file's docstring")
            fleets.append(rec)
            case = (M, Fraction(scale), seed, KV)
            inst += [(case, c["k"]) for c in calls if c["success"]]
    sh = pc.shares(inst)
    print(f"{len(fleets)} fleets, {sh}", file=sys.stderr)
    for key, floor in pc.FLOORS.items():
        assert sh[key] >= floor * sh["feasible"], (key, sh)
    out = {"model": "llama_3_70b/online", "kv_bits": KV, "mip_gap": GAP, "fleets": fleets}
    (HERE / "pressure.json").write_text(json.dumps(out, indent=None, separators=(",", ":")))


if __name__ == "__main__":
    main()
