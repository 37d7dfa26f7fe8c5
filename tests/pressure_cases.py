"""Memory-pressured fleets and their exact-oracle answers, shared by test_pressure.py, test_gpu_pressure.py and
tests/golden/gen_pressure.py.

pressured_fleet(seed, M, scale) is synth_fleet(seed, M) with d_avail_ram, d_avail_metal and d_avail_cuda of
every device multiplied by `scale` and truncated to int; every other field is the unscaled fleet's, so seeds
stay comparable with the rest of the suite. On the 80-layer llama_3_70b/online model (about 0.52 GB a layer at
kv 4bit) the unscaled fleets of 16 and 64 devices never use a slack, a t column or a partial offload in any
optimum; at 1/16 and below nearly every optimum does ("Memory pressure").

A class is (M, scale); a case is (M, scale, seed, kv_bits); an instance is (case, k). The oracle is
oracle/halda_exact.c through mo.exact_solve(mo.lower_dense(...)): it enumerates every (w_i, n_i) and assumes no
convexity. Its answers are computed once per session (lru_cache) and must not be modified by a test.

M = 33 uses scale 1/32 (the issue's first choice; it clears the floors of test_pressure_cases_are_pressured)."""

import sys
from fractions import Fraction
from functools import lru_cache

import numpy as np

from oracle import milp_oracle as mo

L = 80
KS = (1, 2, 4, 5, 8, 10, 16, 20, 40)
REL_OBJ = 1e-9
S16, S32, S64 = Fraction(1, 16), Fraction(1, 32), Fraction(1, 64)

# (M, scale): (seeds at kv 4bit, seeds at kv fp16)
CLASSES = {
    (64, S16): (range(16), range(4)), (64, S64): (range(16), range(4)),
    (16, S16): (range(16), range(4)), (16, S64): (range(16), range(4)),
    (33, S32): (range(8), ()),
    (2, S16): (range(8), ()), (3, S16): (range(8), ()), (5, S16): (range(8), ()),
}
# the k asked of a class: M = 16 the four k with room, M = 33 k = 1, 2, M = 64 k = 1, the small fleets every k
# of 80 with W = 80 // k >= M
CLASS_KS = {64: (1,), 16: (1, 2, 4, 5), 33: (1, 2)}


def ks_of(M):
    return CLASS_KS.get(M, tuple(k for k in KS if L // k >= M))


def cases(Ms=None, kvs=("4bit", "fp16"), seeds=None, scales=None):
    """[(M, scale, seed, kv_bits)] of the case list, optionally narrowed."""
    out = []
    for (M, sc), (s4, s16) in CLASSES.items():
        if (Ms is not None and M not in Ms) or (scales is not None and sc not in scales):
            continue
        for kv, ss in (("4bit", s4), ("fp16", s16)):
            if kv in kvs:
                out += [(M, sc, s, kv) for s in ss if seeds is None or s in seeds]
    return out


def instances(case_list=None):
    """[(case, k)] of every (case, k) asked."""
    return [(c, k) for c in (cases() if case_list is None else case_list) for k in ks_of(c[0])]


@lru_cache(maxsize=None)
def our_model():
    from distilp_amd.common import ModelProfileSplit
    from distilp_amd.synth import load_model_dict

    return ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()


def pressured_fleet(seed, M, scale):
    """synth_fleet(seed, M) as dicts, the three memory fields times `scale`, truncated to int."""
    from distilp_amd.synth import synth_fleet

    dicts = synth_fleet(seed, M)
    for d in dicts:
        for f in ("d_avail_ram", "d_avail_metal", "d_avail_cuda"):
            if d[f] is not None:
                d[f] = int(d[f] * float(scale))
    return dicts


@lru_cache(maxsize=None)
def _devices(seed, M, scale):
    from distilp_amd.common import DeviceProfile

    return tuple(DeviceProfile.model_validate(d) for d in pressured_fleet(seed, M, scale))


def devices(seed, M, scale):
    return list(_devices(seed, M, Fraction(scale)))


def kv_factor(kv_bits):
    return mo._kv_factor(kv_bits)


@lru_cache(maxsize=None)
def problem(case, k):
    """The dense problem of (case, k). Shared: read only."""
    M, sc, s, kv = case
    return mo.lower_dense(devices(s, M, sc), our_model(), k, kv_factor(kv))


@lru_cache(maxsize=None)
def exact(case, k):
    """(status, x, best, second) of the exact oracle on (case, k). Shared: read only."""
    st, x, b1, b2, _ = mo.exact_solve(problem(case, k))
    x.setflags(write=False)
    return st, x, b1, b2


def unique(case, k):
    st, _, b1, b2 = exact(case, k)
    return st == 0 and mo.uniqueness_margin_ok(b1, b2)


def objective(case, k):
    """The oracle's obj_value (c.x + constants) of a feasible (case, k)."""
    return mo.objective_value(problem(case, k), exact(case, k)[1])


def best_k(case, ks=None):
    """(k, obj_value) of the reference's k-sweep (ascending k, strict "<") by the exact oracle, or None."""
    best = None
    for k in sorted(ks_of(case[0]) if ks is None else ks):
        if L // k < case[0] or exact(case, k)[0] != 0:
            continue
        o = objective(case, k)
        if best is None or o < best[1]:
            best = (k, o)
    return best


def traits(case, k):
    """(some s1/s2/s3 > 0, some t > 0, some GPU device with 0 < n_i < w_i) of the oracle's optimum."""
    st, x, _, _ = exact(case, k)
    assert st == 0
    M = case[0]
    p = problem(case, k)
    w, n = np.rint(x[:M]), np.rint(x[M:2 * M])
    gpu = p["ub"][M:2 * M] > 0
    return (bool((x[2 * M:5 * M] > 0.5).any()), bool((x[5 * M:6 * M] > 0.5).any()),
            bool((gpu & (n > 0) & (n < w)).any()))


def shares(inst):
    """{feasible, slack, t, partial, unique}: counts over the instances `inst` ([(case, k)])."""
    out = {"instances": len(inst), "feasible": 0, "slack": 0, "t": 0, "partial": 0, "unique": 0}
    for c, k in inst:
        if exact(c, k)[0] != 0:
            continue
        s, t, part = traits(c, k)
        out["feasible"] += 1
        out["slack"] += s
        out["t"] += t
        out["partial"] += part
        out["unique"] += unique(c, k)
    return out


FLOORS = {"slack": 0.90, "t": 0.25, "partial": 0.25, "unique": 0.95}  # shares of the feasible instances


def close(a, b, rel=REL_OBJ):
    return abs(a - b) <= rel * max(1.0, abs(b))


def check_x(x, case, k, what="", cases=None):
    """Assert a solver's x of (case, k) is the oracle's optimum: c.x within 1e-9 relative and, where the
    optimum is unique, the w, n, s1, s2, s3 and t columns equal to the oracle's. `cases`: the case module whose
    exact / problem / unique look the case up (this one; tests/irregular_cases.py passes itself)."""
    cs = cases or sys.modules[__name__]
    st, xo, b1, _ = cs.exact(case, k)
    assert st == 0, (what, case, k)
    M = case[0]
    p = cs.problem(case, k)
    x = np.asarray(x[:7 * M + 1], np.float64)
    assert close(float(np.dot(p["c"], x)), b1), (what, case, k, float(np.dot(p["c"], x)), b1)
    if cs.unique(case, k):
        assert np.array_equal(x[:2 * M], xo[:2 * M]), (what, case, k, "w / n", x[:2 * M], xo[:2 * M])
        assert np.array_equal(x[2 * M:6 * M], np.rint(xo[2 * M:6 * M])), (
            what, case, k, "slack / t", x[2 * M:6 * M], xo[2 * M:6 * M])


# ------------------------------------------------------------------ tests/golden/pressure.json
def golden_seeds(M):
    """The seeds of a class recorded in pressure.json: 0..3, cut to 0..1 for the fleets of 2, 3 and 5 devices
    -- each of those contributes every k of 80 with room (7 to 9 instances a fleet, against 1 to 4 of the large
    fleets), and with four seeds of them the file's instances miss the slack and t floors (87.5 % and 21.5 %)."""
    return range(4) if M >= 16 else range(2)


REL_LOSING_K = 1.5e-6  # a losing k's recorded objective: HiGHS's primal feasibility tolerance (tests/test_variants.py)


def golden_devices(rec):
    return devices(rec["seed"], rec["M"], Fraction(*rec["scale"]))


def result_mismatch(got, rec, per_k_exact):
    """None when `got` (a dict or HALDAResult-like with k, w, n, obj_value, sets; None = no feasible k) agrees
    with the recorded reference result of `rec` under the standing rule -- objective within 1e-9 relative,
    (k, w, n, sets) identical where the exact oracle's margins exceed 1e-7 -- else what differs."""
    from .subfleets_cases import result_mismatch as rule

    return rule(got, rec, per_k_exact)


def golden_mismatch(rec, solver):
    """oracle.milp_oracle's k-sweep by `solver` ("exact" / "highs") on a recorded fleet against the record:
    None when they agree (status per k, a losing k's objective within 1.5e-6, the result by the standing
    rule), else what differs."""
    return sweep_mismatch(golden_devices(rec), our_model(), rec, solver)


def sweep_mismatch(devs, model, rec, solver):
    """golden_mismatch on any fleet and model (kv 4bit, mip_gap 1e-4)."""
    best, exact_k = mo.halda_solve_oracle(devs, model, mip_gap=1e-4, kv_bits="4bit", solver="exact")
    per_k = exact_k
    if solver != "exact":
        best, per_k = mo.halda_solve_oracle(devs, model, mip_gap=1e-4, kv_bits="4bit", solver=solver)
    ref_k = {r["k"]: r for r in rec["per_k"]}
    if sorted(ref_k) != [r["k"] for r in per_k]:
        return f"k lists differ: {sorted(ref_k)} vs {[r['k'] for r in per_k]}"
    for r in per_k:
        g = ref_k[r["k"]]
        if r["success"] != g["success"]:
            return f"k={r['k']}: success {r['success']} vs reference {g['success']}"
        if r["success"] and not close(r["obj_value"], g["obj_value"], REL_LOSING_K):
            return f"k={r['k']}: obj_value {r['obj_value']!r} vs reference {g['obj_value']!r}"
    return result_mismatch(best, rec, exact_k)


# ------------------------------------------------------------------ neighbour plans (tests/golden/gen_plans.py's)
NEIGHBOUR_SEED = 20261019
# At the scales of the case list no single-layer neighbour of an optimum pushes a slack past its bound W (0 of
# 2,208; nor at 1/32, 1/64 or 1/256 of the 2-, 3-, 5- and 16-device fleets): s <= W binds only on a device with next
# to no memory. Eight 2-device fleets at scale 2^-14 are therefore added to the neighbour plans alone, after the
# case list (whose draws they leave unchanged): their optima sit at the bound and a move onto the head exceeds it.
NEIGHBOUR_EXTRA = tuple((2, Fraction(1, 1 << 14), s, "4bit") for s in range(8))


def neighbours(rng, w, n):
    """Six neighbours of (w, n) drawn as tests/golden/gen_plans.py draws them: (kind, w', n')."""
    from tests.golden.gen_plans import neighbours as gen

    return gen(rng, list(w), list(n))


@lru_cache(maxsize=None)
def neighbour_plans():
    """[(case, k, kind, w, n)]: the oracle's optimum of every kv 4bit instance ("optimum") and its six
    neighbours, one fixed-seed stream over the case list in order, then over NEIGHBOUR_EXTRA."""
    rng = np.random.default_rng(NEIGHBOUR_SEED)
    out = []
    for c, k in instances(cases(kvs=("4bit",))) + instances(list(NEIGHBOUR_EXTRA)):
        st, x, _, _ = exact(c, k)
        if st != 0:
            continue
        M = c[0]
        w = [int(round(v)) for v in x[:M]]
        n = [int(round(v)) for v in x[M:2 * M]]
        out.append((c, k, "optimum", w, n))
        out += [(c, k, kind, w2, n2) for kind, w2, n2 in neighbours(rng, w, n)]
    return out


def price_fixed(case, k, w, n, prob=None):
    """(success, obj_value or None) of HiGHS on (case, k) with the w and n columns fixed to the plan. `prob`: the
    dense problem, when the case is another module's."""
    p = dict(problem(case, k) if prob is None else prob)
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
