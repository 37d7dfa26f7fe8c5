"""Shared by test_subsets.py and test_gpu_subsets.py: the case lists of exact device selection and the
brute force over the exact oracle (oracle/halda_exact.c through mo.halda_solve_oracle) that specifies it.

A case is (seed, M, max_drop or None, keep): the synthetic fleet (seed, M) of subfleets_cases.our_devices on
the 80-layer model, default k list, kv 8bit. The oracle's answers are computed once per session (lru_cache)
and must not be modified by a test."""

import itertools
import math
from fractions import Fraction
from functools import lru_cache

from oracle import milp_oracle as mo

from .subfleets_cases import our_devices, our_model

REL_OBJ = 1e-9  # the project's parity tolerance on the objective

# host selection logic (test_subsets.py): all subsets of M = 3 .. 6, and M = 8 with D = 2
HOST_CASES = [(9100 + M, M, None, ()) for M in (3, 4, 5, 6)] + [(9108, 8, 2, ()), (9205, 5, None, (0,)),
                                                                 (9306, 6, 3, (1, 4))]
# the Python entries on the GPU against the brute force (test_gpu_subsets.py). The near-tie share of these
# seeds, by the oracle alone, is checked on the CPU (test_subsets.py::test_near_ties_stay_inside_the_cap)
ENTRY_CASES = [(9100 + M, M, None, ()) for M in (3, 4, 5, 6)] + [(9205, 5, None, (0,)), (9108, 8, 2, ())]
NEAR_TIE_CAP = 0.25

# bit identity per candidate on both routes: (seed, M, max_drop or None)
IDENTITY_CASES = [(9103, 3, None), (9105, 5, None), (9106, 6, None), (9116, 16, 2)]

# a memory-starved fleet (pressure_cases.pressured_fleet) one of whose devices cannot serve the model alone:
# with that device kept, the group d = M - 1 (that device alone) has no feasible candidate
STARVED = (3, 3, Fraction(1, 1024))  # (seed, M, scale)


@lru_cache(maxsize=None)
def starved_keep():
    """The device of the STARVED fleet whose one-device sub-fleet is infeasible by the exact oracle."""
    from . import pressure_cases as pc

    seed, M, scale = STARVED
    devs = pc.devices(seed, M, scale)
    alone = [mo.halda_solve_oracle([d], pc.our_model(), mip_gap=1e-4, kv_bits="8bit", solver="exact")[0]
             for d in devs]
    dead = [i for i, r in enumerate(alone) if r is None]
    assert len(dead) == 1, alone
    return dead[0]


# A fleet key names a device list: ("synth", seed, M) -- subfleets_cases.our_devices, kv 8bit, the default k list --
# ("p", M, scale, seed) a pressured fleet and ("i", irregular case) an edited one, both kv 4bit on the k of PRESSURE_KS;
# ("deep", M, seed, L, ks) bounds_cases.devices(M, seed) on the model with L layers, kv 4bit, on the k list ks.
PRESSURE_KS = {5: None, 16: (1, 2, 4, 5), 64: (1,)}  # None: the default k list


def fleet_of(key):
    """(devs, model, kv_bits, k_candidates or None) of a fleet key."""
    if key[0] == "synth":
        return our_devices(key[1], key[2]), our_model(), "8bit", None
    from . import irregular_cases as ic
    from . import pressure_cases as pc

    if key[0] == "deep":  # ("deep", M, seed, L, k list or None): bounds_cases.devices(M, seed) on the model at L
        from . import bounds_cases as bc

        _, M, seed, L, ks = key
        return list(bc.devices(M, seed)), pc.our_model().model_copy(update={"L": L}), "4bit", ks
    if key[0] == "p":
        _, M, scale, seed = key
        return pc.devices(seed, M, scale), pc.our_model(), "4bit", PRESSURE_KS[M]
    case = key[1]
    assert ic.model_of(case) is pc.our_model()
    return ic.devices(case), pc.our_model(), "4bit", PRESSURE_KS[case[0]]


@lru_cache(maxsize=None)
def oracle_of(key, kept):
    """The exact oracle's result dict (None: infeasible) of the sub-fleet `kept` (a tuple of indices) of a fleet
    key; kappa's head is the kept list's first is_head device, else its first device."""
    devs, model, kv, ks = fleet_of(key)
    best, _ = mo.halda_solve_oracle([devs[i] for i in kept], model, k_candidates=ks, mip_gap=1e-4, kv_bits=kv,
                                    solver="exact")
    return best


def oracle_list(seed, M, kept, kv_bits="8bit"):
    """oracle_of on the synthetic fleet (seed, M)."""
    assert kv_bits == "8bit"
    return oracle_of(("synth", seed, M), tuple(kept))


def slots_of(M, keep):
    return [i for i in range(M) if i not in set(keep)]


def limit_of(M, keep, max_drop):
    lim = min(len(slots_of(M, keep)), M - 1)
    return lim if max_drop is None else min(max_drop, lim)


def candidates(M, keep, d):
    """[(dropped, kept)] with d drops in enumeration order."""
    return [(c, tuple(i for i in range(M) if i not in c)) for c in itertools.combinations(slots_of(M, keep), d)]


def brute_force(seed, M, max_drop, keep):
    """brute_force_of on the synthetic fleet (seed, M)."""
    return brute_force_of(("synth", seed, M), max_drop, keep)


def brute_force_of(key, max_drop, keep):
    """Per d: (best obj or inf, dropped of the earliest minimum or None, runner-up obj or inf) by the oracle."""
    out = []
    M = len(fleet_of(key)[0])
    for d in range(limit_of(M, keep, max_drop) + 1):
        objs = []
        for gone, kept in candidates(M, keep, d):
            r = oracle_of(key, kept)
            objs.append((math.inf if r is None else r["obj_value"], gone))
        best = min(objs, key=lambda t: t[0])  # min keeps the earliest among equals
        others = sorted(o for o, g in objs if g != best[1])
        out.append((best[0], best[1] if best[0] < math.inf else None, others[0] if others else math.inf))
    return out


def _pressure_cases():
    """(key, max_drop or None, keep) under memory pressure and with moved heads: three pressured 5-device fleets,
    every subset; a pressured 16-device fleet at D = 2; 16-device fleets with two heads, the head last and no head,
    D = 2, without `keep` and with `keep` naming the head (device 0 where there is none); and a pressured and a
    head-last 64-device fleet at D = 1 (the fused route)."""
    from . import irregular_cases as ic
    from . import pressure_cases as pc

    out = [(("p", 5, pc.S16, s), None, ()) for s in range(3)] + [(("p", 16, pc.S16, 0), 2, ())]
    for edit in ("two_heads", "head_at:last", "no_head"):
        case = (16, pc.S16, 1, "4bit", (edit,))
        head = ic.head_of(ic.edited_fleet(1, 16, pc.S16, (edit,))[0])
        out += [(("i", case), 2, ()), (("i", case), 2, (head,))]
    out += [(("p", 64, pc.S16, 0), 1, ()), (("i", (64, pc.S16, 0, "4bit", ("head_at:last",))), 1, ())]
    return out


PRESSURE_CASES = _pressure_cases()


def oracle_solver(seed, M):
    """A `_solve_lists` hook backed by the oracle: results carry obj_value, k, w, n and the kept list."""
    import types

    def solve(lists):
        out = []
        for s in lists:
            r = oracle_list(seed, M, tuple(s))
            out.append(None if r is None else types.SimpleNamespace(obj_value=r["obj_value"], k=r["k"], w=r["w"],
                                                                    n=r["n"], kept=list(s)))
        return out

    return solve


def near_tie(best, runner):
    return not abs(runner - best) > REL_OBJ * max(1.0, abs(best))
