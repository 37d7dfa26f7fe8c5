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


@lru_cache(maxsize=None)
def oracle_list(seed, M, kept, kv_bits="8bit"):
    """The exact oracle's result dict (None: infeasible) of the sub-fleet `kept` (a tuple of indices)."""
    devs = our_devices(seed, M)
    best, _ = mo.halda_solve_oracle([devs[i] for i in kept], our_model(), mip_gap=1e-4, kv_bits=kv_bits,
                                    solver="exact")
    return best


def slots_of(M, keep):
    return [i for i in range(M) if i not in set(keep)]


def limit_of(M, keep, max_drop):
    lim = min(len(slots_of(M, keep)), M - 1)
    return lim if max_drop is None else min(max_drop, lim)


def candidates(M, keep, d):
    """[(dropped, kept)] with d drops in enumeration order."""
    return [(c, tuple(i for i in range(M) if i not in c)) for c in itertools.combinations(slots_of(M, keep), d)]


def brute_force(seed, M, max_drop, keep):
    """Per d: (best obj or inf, dropped of the earliest minimum or None, runner-up obj or inf) by the oracle."""
    out = []
    for d in range(limit_of(M, keep, max_drop) + 1):
        objs = []
        for gone, kept in candidates(M, keep, d):
            r = oracle_list(seed, M, kept)
            objs.append((math.inf if r is None else r["obj_value"], gone))
        best = min(objs, key=lambda t: t[0])  # min keeps the earliest among equals
        others = sorted(o for o, g in objs if g != best[1])
        out.append((best[0], best[1] if best[0] < math.inf else None, others[0] if others else math.inf))
    return out


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
