"""Shared by test_subfleets.py, test_gpu_subfleets.py and tests/golden/gen_golden_subfleets.py: the synthetic
fleets behind tests/golden/subfleets.json and the suite's standing parity rule against recorded reference
results -- identical status; objective within 1e-9 relative; identical (k, w, n, sets) where the exact
oracle's margin exceeds 1e-7 relative (the optimum and the best k are then unique)."""

from functools import lru_cache

from oracle import milp_oracle as mo

REL_OBJ, REL_MARGIN = 1e-9, 1e-7


@lru_cache(maxsize=None)
def our_model():
    from distilp_amd.common import ModelProfileSplit
    from distilp_amd.synth import load_model_dict

    return ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()


@lru_cache(maxsize=None)
def _fleet(seed, M):
    from distilp_amd.common import DeviceProfile
    from distilp_amd.synth import synth_fleet

    return tuple(DeviceProfile.model_validate(d) for d in synth_fleet(seed, M))


def our_devices(seed, M, drop=None):
    """The synthetic fleet (seed, M), without device `drop` when given."""
    devs = list(_fleet(seed, M))
    return devs if drop is None else devs[:drop] + devs[drop + 1:]


def close(a, b, rel=REL_OBJ):
    return abs(a - b) <= rel * max(1.0, abs(b))


@lru_cache(maxsize=None)
def exact_sweep(seed, M, drop, kv_bits):
    """The exact oracle's k-sweep of one leave-one-out list, computed once per session."""
    return mo.halda_solve_oracle(our_devices(seed, M, drop), our_model(), mip_gap=1e-4, kv_bits=kv_bits,
                                 solver="exact")


def unique_optimum(per_k_exact, k_best):
    """Whether the exact oracle proves (k, w, n) unique: the best k's own second-best margin, and its
    distance to every other k's optimum, exceed 1e-7 relative."""
    by_k = {r["k"]: r for r in per_k_exact if r["success"]}
    b = by_k[k_best]
    tol = REL_MARGIN * max(1.0, abs(b["obj_value"]))
    return b["margin"] > tol and all(abs(r["obj_value"] - b["obj_value"]) > tol for k, r in by_k.items() if k != k_best)


def result_mismatch(got, rec, per_k_exact):
    """None when `got` (a dict or HALDAResult-like with k, w, n, obj_value, sets; None = infeasible) agrees
    with the recorded reference result `rec["result"]` under the rule above, else what differs."""
    ref = rec["result"]
    if ref is None or got is None:
        return None if ref is None and got is None else f"feasibility: got {got}, reference {ref}"
    g = got if isinstance(got, dict) else {f: getattr(got, f) for f in ("k", "w", "n", "obj_value", "sets")}
    if not close(g["obj_value"], ref["obj_value"]):
        return f"obj_value {g['obj_value']!r} vs reference {ref['obj_value']!r}"
    if unique_optimum(per_k_exact, ref["k"]):
        a, b = (g["k"], g["w"], g["n"], g["sets"]), (ref["k"], ref["w"], ref["n"], ref["sets"])
        if a != b:
            return f"(k, w, n, sets) {a} vs reference {b}"
    return None


def golden_mismatch(devs, model, rec, kv_bits="8bit"):
    """The exact oracle on `devs` against one recorded leave-one-out case (its result and every k): None
    when they agree under the rule above, else what differs."""
    best, per_k = mo.halda_solve_oracle(devs, model, mip_gap=1e-4, kv_bits=kv_bits, solver="exact")
    ref_k = {r["k"]: r for r in rec["per_k"]}
    if sorted(ref_k) != [r["k"] for r in per_k]:
        return f"k lists differ: {sorted(ref_k)} vs {[r['k'] for r in per_k]}"
    for r in per_k:
        g = ref_k[r["k"]]
        if r["success"] != g["success"]:
            return f"k={r['k']}: success {r['success']} vs reference {g['success']}"
        if not r["success"]:
            continue
        if not close(r["obj_value"], g["obj_value"]):
            return f"k={r['k']}: obj_value {r['obj_value']!r} vs reference {g['obj_value']!r}"
        if r["margin"] > REL_MARGIN * max(1.0, abs(r["obj_value"])) and (r["w"], r["n"]) != (g["w"], g["n"]):
            return f"k={r['k']}: (w, n) {(r['w'], r['n'])} vs reference {(g['w'], g['n'])}"
    return result_mismatch(best, rec, per_k)
