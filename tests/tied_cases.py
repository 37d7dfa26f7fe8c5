"""Homogeneous and duplicated fleets at the sizes of every GPU route, and their exact-oracle answers, shared by
test_tied.py and test_gpu_tied.py.

The three kinds of tests/ties.py (copies, two, half) widened to M devices: the devices are drawn from
synth_fleet(seed, max(M, 16)) or, with a memory scale, from pressure_cases.pressured_fleet(seed, max(M, 16), scale)
before they are repeated, and picked as tied_fleets picks them. On such a fleet the optimum is almost never unique,
so the solver's tie rules decide which optimal plan comes back; the check here (check_plan) therefore does not lean
on uniqueness: it re-prices the returned (w, n) with the exact oracle, both column groups pinned.

A class is a row of CLASSES; a case is (class, kind, scale, seed), always at kv 4bit; an instance is (case, k) with
room (L // k >= M). The oracle is oracle/halda_exact.c through mo.exact_solve; its answers are computed once per
session (lru_cache) and must not be modified by a test."""

import copy
from fractions import Fraction
from functools import lru_cache

import numpy as np

from oracle import milp_oracle as mo

from . import pressure_cases as pc
from .ties import KINDS, tied_dicts

SEED0 = 21000
KV_BITS = "4bit"
KV = 0.5
REL_OBJ = pc.REL_OBJ
S1, S16, S64 = Fraction(1), pc.S16, pc.S64
KS160 = (1, 2, 4, 5, 8, 10, 16, 20, 32, 40, 80)

# class: (M, L, the k asked, scales, seeds)
CLASSES = {
    "T64": (64, 80, pc.KS, (S1, S16, S64), (21000, 21005)),
    "T33": (33, 80, (1, 2), (S1, S16, S64), (21000, 21005)),
    "T16p": (16, 80, (1, 2, 4, 5), (S16, S64), (21000, 21005)),
    "T70": (70, 80, (1,), (S1, S64), (21000,)),
    "D64": (64, 160, (1, 2), (S1, S64), (21000,)),
}
FRONTIER_RUNS = (("T16p", 1), ("T16p", 2), ("T64", 1))  # the (class, k) of the move frontier test (P = 4)


def M_of(case):
    return CLASSES[case[0]][0]


def L_of(case):
    return CLASSES[case[0]][1]


def sweep_ks(cls):
    """The k list a sweep of the class runs over: every factor used of its L (a k without room is infeasible)."""
    return list(pc.KS if CLASSES[cls][1] == 80 else KS160)


def class_ks(cls):
    """The k asked of a class that have room."""
    M, L, ks, _, _ = CLASSES[cls]
    return tuple(k for k in ks if L // k >= M)


def ks_of(case):
    """The k asked of the case's class that have room."""
    return class_ks(case[0])


def cases(cls, kinds=None, scales=None, seeds=None):
    """[(class, kind, scale, seed)] of a class in the list's order (kind, then scale, then seed), narrowed."""
    _, _, _, scs, sds = CLASSES[cls]
    return [(cls, kind, sc, s) for kind in KINDS for sc in scs for s in sds
            if (kinds is None or kind in kinds) and (scales is None or sc in scales) and (seeds is None or s in seeds)]


def all_cases():
    return [c for cls in CLASSES for c in cases(cls)]


def instances(case_list=None):
    return [(c, k) for c in (all_cases() if case_list is None else case_list) for k in ks_of(c)]


def kslot_batch():
    """The T16p cases six times over (72 fleets): the k-slot kernel takes batches of more than 64 fleets."""
    return cases("T16p") * 6


def mixed_batch():
    """One mixed-size batch: the T64, T33, T16p and T70 cases taken in turn."""
    groups = [cases(cls) for cls in ("T64", "T33", "T16p", "T70")]
    out = []
    for i in range(max(len(g) for g in groups)):
        out += [g[i] for g in groups if i < len(g)]
    return out


@lru_cache(maxsize=None)
def model(L=80):
    m = pc.our_model()
    return m if L == m.L else m.model_copy(update={"L": L})


def model_of(case):
    return model(L_of(case))


@lru_cache(maxsize=None)
def _devices(case):
    from distilp_amd.common import DeviceProfile
    from distilp_amd.synth import synth_fleet

    cls, kind, scale, seed = case
    M = M_of(case)
    src = synth_fleet(seed, max(M, 16)) if scale == 1 else pc.pressured_fleet(seed, max(M, 16), scale)
    return tuple(DeviceProfile.model_validate(copy.deepcopy(d)) for d in tied_dicts(kind, src, seed - SEED0, M))


def devices(case):
    return list(_devices(case))


@lru_cache(maxsize=None)
def problem(case, k):
    """The dense problem of (case, k). Shared: read only."""
    return mo.lower_dense(devices(case), model_of(case), k, KV)


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


def plan_of(case, k):
    """(w, n) of the oracle's optimum as int lists."""
    x, M = exact(case, k)[1], M_of(case)
    return [int(round(v)) for v in x[:M]], [int(round(v)) for v in x[M:2 * M]]


def best_k(case, ks=None):
    """(k, obj_value) of the reference's k-sweep (ascending k, strict "<") by the exact oracle, or None."""
    best = None
    for k in sorted(ks_of(case) if ks is None else ks):
        if L_of(case) // k < M_of(case) or exact(case, k)[0] != 0:
            continue
        o = objective(case, k)
        if best is None or o < best[1]:
            best = (k, o)
    return best


def best_k_decided(case, ks=None):
    """False where the two best objectives over k are within 1e-7 relative: the best-k comparison is skipped."""
    objs = sorted(objective(case, k) for k in (ks_of(case) if ks is None else ks)
                  if L_of(case) // k >= M_of(case) and exact(case, k)[0] == 0)
    return len(objs) < 2 or objs[1] - objs[0] > 1e-7 * max(1.0, abs(objs[0]))


def traits(case, k):
    """(some s1/s2/s3 > 0, some GPU device with 0 < n_i < w_i) of the oracle's optimum."""
    x, M = exact(case, k)[1], M_of(case)
    w, n = np.rint(x[:M]), np.rint(x[M:2 * M])
    return bool((x[2 * M:5 * M] > 0.5).any()), bool(((n > 0) & (n < w)).any())


close = pc.close


def pinned_problem(prob, w, n):
    """`prob` with the w and n columns' bounds set to the plan, or None where the plan leaves the bounds."""
    M = prob["M"]
    v = np.asarray(list(w) + list(n), float)
    if len(v) != 2 * M or (v < prob["lb"][:2 * M]).any() or (v > prob["ub"][:2 * M]).any():
        return None
    q = dict(prob)
    q["lb"], q["ub"] = prob["lb"].copy(), prob["ub"].copy()
    q["lb"][:2 * M] = v
    q["ub"][:2 * M] = v
    return q


def price(prob, w, n):
    """The exact oracle on `prob` with both column groups pinned to (w, n): obj_value, or None (infeasible)."""
    q = pinned_problem(prob, w, n)
    if q is None:
        return None
    st, x, _, _, _ = mo.exact_solve(q)
    return mo.objective_value(q, x) if st == 0 else None


_PRICES = {}


def pinned_price(case, k, w, n):
    """The least objective of (case, k) at the plan (w, n), by the exact oracle; None when the plan is infeasible.
    Kept per plan: the routes return the same few plans many times over."""
    key = (case, k, tuple(int(v) for v in w), tuple(int(v) for v in n))
    if key not in _PRICES:
        _PRICES[key] = price(problem(case, k), key[2], key[3])
    return _PRICES[key]


def check_plan(case, k, w, n, obj, what=""):
    """Assert (w, n) is an optimal plan of (case, k) and `obj` its objective, without leaning on uniqueness:
    sum w = L // k; the plan is feasible and its best completion prices at the oracle's optimum within 1e-9
    relative; the reported objective is within 1e-9 of the same; where the optimum is unique, (w, n) is it."""
    st = exact(case, k)[0]
    assert st == 0, (what, case, k, st)
    M = M_of(case)
    w, n = [int(v) for v in w], [int(v) for v in n]
    assert len(w) == M and len(n) == M, (what, case, k)
    assert sum(w) == L_of(case) // k, (what, case, k, sum(w))
    want = objective(case, k)
    got = pinned_price(case, k, w, n)
    assert got is not None, (what, case, k, "infeasible plan", w, n)
    assert close(got, want), (what, case, k, "plan prices at", got, "optimum", want, w, n)
    assert close(float(obj), want), (what, case, k, "reported", float(obj), "optimum", want)
    if unique(case, k):
        assert (w, n) == plan_of(case, k), (what, case, k, (w, n), plan_of(case, k))


def check_x(case, k, x, obj, what=""):
    """check_plan on the w / n columns of a dense x."""
    M = M_of(case)
    check_plan(case, k, np.rint(x[:M]), np.rint(x[M:2 * M]), obj, what)


# ------------------------------------------------------------------ the stale placement of the bounded / budget tests
def roll_of(case):
    """How far the oracle's optimal w is rolled to make w0, chosen so that every class has a case within P = 4
    loaded layers of the optimum (test_tied.py): one device on `copies` and `two` fleets -- on `two` only the two
    devices at the ends of the groups then hold another device's layers, where a roll by floor(M/2), each half
    holding the other's plan, is 8 to 96 layers away --, and ceil(M/2) on a `half` fleet: every device holds its
    twin's layers, where a roll by one is up to 96 layers away."""
    return -(-M_of(case) // 2) if case[1] == "half" else 1


def rolled_w0(case, k):
    w, _ = plan_of(case, k)
    return [int(v) for v in np.roll(w, roll_of(case))]


def p_star(case, k):
    """sum max(0, w*_i - w0_i) for the oracle's optimum w* and w0 = rolled_w0: the loads that reach it from w0."""
    w, _ = plan_of(case, k)
    return sum(max(0, a - b) for a, b in zip(w, rolled_w0(case, k)))
