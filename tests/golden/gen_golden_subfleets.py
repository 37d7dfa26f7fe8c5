"""Generate tests/golden/subfleets.json from the REFERENCE implementation (this container only).

Run:  python tests/golden/gen_golden_subfleets.py      (needs /root/reference; under a minute)

The reference is imported exactly as gen_golden.py imports it (its import_reference / run_solve). For
synthetic fleets (distilp_amd.synth.synth_fleet(seed, M), the llama_3_70b/online model) of 2, 3, 8 and 16
devices the file holds the reference's `halda_solve` (kv 8bit, the default mip_gap 1e-4) on EVERY
leave-one-out list `devs[:i] + devs[i + 1:]` -- the list without device 0 has no is_head device -- as
recorded results only: the HALDAResult fields and, per k, success / w / n / obj_value. The device dicts are
not stored (synth_fleet regenerates them from the seed).

Every recorded case is checked here against the exact oracle under the suite's standing rule
(tests/subfleets_cases.py: status, objective within 1e-9 relative, (k, w, n, sets) where the exact margin
exceeds 1e-7). A disagreement STOPS the generator: it is either a bug on this side, which the tests must
show, or the reference's HiGHS disagreeing with itself (the reference_unstable class of DESIGN.md §9),
which a person establishes on the reference alone before adding the fleet's seed to UNSTABLE_SEEDS below;
such a seed is replaced by the next one and recorded under "replaced_seeds". No case of a kept fleet is
skipped. UNSTABLE_SEEDS is empty: no seed had to be replaced.
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path.append(str(REPO))

SIZES = {2: 3, 3: 3, 8: 2, 16: 2}  # M: fleets
SEED0 = 7000
KV, GAP = "8bit", 1e-4
UNSTABLE_SEEDS = {}  # (M, seed): how the reference was shown to disagree with itself


def main():
    from gen_golden import import_reference, run_solve

    hp, _, DeviceProfile, ModelProfileSplit = import_reference()
    from distilp_amd.synth import load_model_dict, synth_fleet
    from tests.subfleets_cases import golden_mismatch, our_model, our_devices

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    fleets, replaced = [], []
    for M, count in SIZES.items():
        seed = SEED0 + 100 * M
        kept = 0
        while kept < count:
            if (M, seed) in UNSTABLE_SEEDS:
                replaced.append({"M": M, "seed": seed, "why": UNSTABLE_SEEDS[(M, seed)]})
                seed += 1
                continue
            dicts = synth_fleet(seed, M)
            lists = []
            for i in range(M):
                sub = [DeviceProfile.model_validate(d) for j, d in enumerate(dicts) if j != i]
                res, err, calls, _ = run_solve(hp, sub, model, KV, GAP)
                rec = {"drop": i, "result": res, "error": err,
                       "per_k": [{k: c[k] for k in ("k", "success", "w", "n", "obj_value") if k in c} for c in calls]}
                why = golden_mismatch(our_devices(seed, M, i), our_model(), rec)
                if why:
                    raise SystemExit(f"M={M} seed={seed} drop={i}: the exact oracle and the reference disagree "
                                     f"({why}); see this file's docstring")
                lists.append(rec)
            fleets.append({"M": M, "seed": seed, "lists": lists})
            kept += 1
            seed += 1
    out = {"model": "llama_3_70b/online", "kv_bits": KV, "mip_gap": GAP, "fleets": fleets, "replaced_seeds": replaced}
    (HERE / "subfleets.json").write_text(json.dumps(out, indent=None, separators=(",", ":")))
    print(f"{len(fleets)} fleets, {sum(len(f['lists']) for f in fleets)} lists, replaced {replaced}", file=sys.stderr)


if __name__ == "__main__":
    main()
