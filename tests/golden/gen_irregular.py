"""Generate tests/golden/irregular.json from the REFERENCE implementation (this container only).

Run:  python tests/golden/gen_irregular.py      (needs the reference checkout that gen_golden.py imports; a few seconds)

The reference is imported exactly as gen_golden.py imports it (its import_reference / run_solve). For every
case of tests/irregular_cases.py with at most 16 devices (golden_cases: every device, head and model edit
occurs among them) the file holds the reference's `halda_solve` (kv 4bit, mip_gap 1e-4, its own k list) on the
edited fleet and model as recorded results only: the HALDAResult fields and, per k, success / w / n /
obj_value; where the reference raises, the exception's type and message instead. The device dicts are not
stored (irregular_cases.edited_fleet regenerates them).

Every recorded fleet is checked here against the exact oracle under the suite's standing rule (same status per
k; the result's objective within 1e-9 relative and its (k, w, n, sets) identical where the exact margin exceeds
1e-7; a losing k's objective within 1.5e-6, tests/test_variants.py). A disagreement STOPS the generator, as in
gen_pressure.py.
"""

from __future__ import annotations

import json
import sys
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
    from tests import irregular_cases as ic

    base = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    fleets = []
    for case in ic.golden_cases():
        M, scale, seed, _, edits = case
        model = ic.edited_model(base, case)
        devs = [DeviceProfile.model_validate(d) for d in ic.edited_fleet(seed, M, scale, edits)[0]]
        res, err, calls, _ = run_solve(hp, devs, model, KV, GAP)
        rec = {"M": M, "scale": [scale.numerator, scale.denominator], "seed": seed, "edits": list(edits),
               "result": res, "error": err,
               "per_k": [{k: c[k] for k in ("k", "success", "w", "n", "obj_value") if k in c} for c in calls]}
        if err is None:
            why = ic.golden_mismatch(rec, "exact")
            if why:
                raise SystemExit(f"{case}: the exact oracle and the reference disagree ({why}); see this file's "
                                 "docstring")
        fleets.append(rec)
    print(f"{len(fleets)} fleets, {sum(f['error'] is not None for f in fleets)} raised", file=sys.stderr)
    out = {"model": "llama_3_70b/online", "kv_bits": KV, "mip_gap": GAP, "fleets": fleets}
    (HERE / "irregular.json").write_text(json.dumps(out, indent=None, separators=(",", ":")))


if __name__ == "__main__":
    main()
