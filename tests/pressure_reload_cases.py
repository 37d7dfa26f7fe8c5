"""The reload-time frontier on memory-pressured fleets and its exact-oracle answers, shared by test_pressure_reload.py,
test_gpu_pressure_reload.py and tests/golden/gen_pressure_scale.py (which asserts the condition below).

test_gpu_boxes.py runs halda_reload_frontier on bounds_cases.devices, where the points of a w_max ladder differ only
in w. On a pressured fleet a device's slack and t change with every rung. The fleets are pressure_cases' (5, 1/16) at
k = 2, (16, 1/64) at k = 2 and (64, 1/16) at k = 1, the incumbent STALE (the optimum of seed + 100 of the class), the
ladder cut after MAX_POINTS points.

The oracle, per point j: mo.exact_solve on a copy of pc.problem with ub[:M] = w0 + caps[j], caps from
boxes.reload_caps (NumPy, no GPU); then the strict running minimum along j. Answers are computed once per session."""

from functools import lru_cache

import numpy as np

from distilp_amd.solver.boxes import reload_caps
from oracle import milp_oracle as mo

from . import pressure_cases as pc
from .pressure_scale_cases import stale_w

MAX_POINTS = 8
FLEETS = ((5, pc.S16, 2, 0), (16, pc.S64, 2, 0), (64, pc.S16, 1, 0))  # (M, scale, k, seed)


def case_of(fleet):
    M, sc, _, s = fleet
    return (M, sc, s, "4bit")


def incumbent(fleet):
    M, sc, k, s = fleet
    return stale_w(M, sc, k, s)


def devices(fleet):
    M, sc, _, s = fleet
    return pc.devices(s, M, sc)


@lru_cache(maxsize=None)
def ladder(fleet):
    """(t, caps) of the fleet's cut ladder."""
    W = pc.L // fleet[2]
    return reload_caps(incumbent(fleet), [float(d.s_disk) for d in devices(fleet)], W, MAX_POINTS)


@lru_cache(maxsize=None)
def raw_points(fleet):
    """Per point j (obj_value or None, x or None) of the exact oracle inside w_max = w0 + caps[j]."""
    M, k = fleet[0], fleet[2]
    base = pc.problem(case_of(fleet), k)
    w0 = np.asarray(incumbent(fleet), float)
    out = []
    for row in ladder(fleet)[1]:
        p = dict(base)
        p["lb"], p["ub"] = base["lb"].copy(), base["ub"].copy()
        p["ub"][:M] = w0 + row
        st, x, _, _, _ = mo.exact_solve(p)
        if st != 0:
            out.append((None, None))
            continue
        x = np.asarray(x, float)
        x.setflags(write=False)
        out.append((mo.objective_value(p, x), x))
    return tuple(out)


def frontier(fleet):
    """[obj_value or None] per point: the strict running minimum of raw_points along j."""
    out, best = [], None
    for o, _ in raw_points(fleet):
        if o is not None and (best is None or o < best):
            best = o
        out.append(best)
    return out


def slack_steps(fleet):
    """The j whose raw optimum differs from point j + 1's in an s1 / s2 / s3 or t column."""
    M, pts = fleet[0], raw_points(fleet)
    return [j for j in range(len(pts) - 1) if pts[j][1] is not None and pts[j + 1][1] is not None
            and not np.array_equal(np.rint(pts[j][1][2 * M:6 * M]), np.rint(pts[j + 1][1][2 * M:6 * M]))]
