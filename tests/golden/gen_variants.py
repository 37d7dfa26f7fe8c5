"""Generate tests/golden/variants.json from the REFERENCE implementation (this container only).

Run:  python tests/golden/gen_variants.py      (needs the reference checkout gen_golden.py names; ~1 minute)

The reference is imported exactly as gen_golden.py imports it (its import_reference / run_solve). For the
fixture folders FOLDERS (devices sorted by file name, device 0 made the head, the decode-phase model: the
CLI's loading) the file holds the reference's own `halda_solve` (default mip_gap 1e-4) on the model with
n_kv replaced by each value of N_KV, at each KV precision of KV: recorded results only -- the HALDAResult
fields and, per k, success / w / n / obj_value.

N_KV is chosen so that the grid is not vacuous: each folder's golden holds at least two different (k, w)
(a scan of n_kv = 2^8 .. 2^22 on the reference: llama_3_70b/online moves from k = 2 through k = 4 and 5 to
k = 1 between 2^10 and 2^20; hermes_70b's single device keeps (40, [2]) up to 2^16 and turns to (1, [80])
from 2^18 at fp16). The generator asserts it, and tests/test_variants.py asserts it on the file.
"""

from __future__ import annotations

import glob
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path.append(str(REPO))

FOLDERS = ["llama_3_70b/online", "hermes_70b"]
KV = ["4bit", "8bit", "fp16"]
N_KV = [512, 65536, 262144, 1048576]
GAP = 1e-4


def main():
    from gen_golden import import_reference, run_solve

    hp, _, DeviceProfile, ModelProfileSplit = import_reference()
    folders = {}
    for folder in FOLDERS:
        base = REPO / "test" / "profiles" / folder
        files = sorted(f for f in glob.glob(str(base / "*.json")) if not f.endswith("model_profile.json"))
        devs = [DeviceProfile.model_validate(json.loads(Path(f).read_text())) for f in files]
        devs[0].is_head = True
        model = ModelProfileSplit.model_validate(json.loads((base / "model_profile.json").read_text())).to_model_profile()
        cases = []
        for n_kv in N_KV:
            m = model.model_copy(update={"n_kv": n_kv})
            for kv in KV:
                res, err, calls, _ = run_solve(hp, devs, m, kv, GAP)
                cases.append({"n_kv": n_kv, "kv_bits": kv, "result": res, "error": err,
                              "per_k": [{k: c[k] for k in ("k", "success", "w", "n", "obj_value") if k in c}
                                        for c in calls]})
        plans = {(c["result"]["k"], tuple(c["result"]["w"])) for c in cases if c["result"]}
        assert len(plans) >= 2, f"{folder}: one plan {plans} over the whole grid -- choose other n_kv"
        folders[folder] = cases
    out = {"mip_gap": GAP, "kv_bits": KV, "n_kv": N_KV, "folders": folders}
    (HERE / "variants.json").write_text(json.dumps(out, indent=None, separators=(",", ":")))
    print({f: len(c) for f, c in folders.items()}, file=sys.stderr)


if __name__ == "__main__":
    main()
