"""The scale-in / scale-out cases and their oracle answers, shared by test_scale.py, test_gpu_scale.py and
tests/golden/gen_scale.py.

Scale-in: the parents of change_cases.LIST_S (4 and 5 devices, k in {1, 2}, a STALE incumbent, so that releases
matter at k = 1 as well) with every PAIR of devices lost (d = 2) on the budgets PS; a pair's frontier is the change
frontier of the three or four survivors holding the incumbent's layers, by change_cases' oracle (a) checked against
(b). Row d = 1 needs no new record: cell (1, p) is the minimum over `lost` of tests/golden/change.json's list S.
Scale-out: a 4-device fleet on its own exact optimum at k = 1 and a pool of 3, a <= 2 devices added, by oracle (a).

tests/golden/scale.json holds the answers (recorded results only)."""

import itertools
import json

from . import bounds_cases as bc
from . import change_cases as cc
from .conftest import GOLDEN

PARENTS = cc.LIST_S
# Further stale parents, the seeds searched so that every (M, k) group has a d = 2 cell whose exact winner is
# strictly better than the pair a greedy repeat of the best single loss picks (gen_scale.py asserts it). Among the
# seeds 0 .. 39 of M = 5 at k = 1 no parent has such a cell; NO_GAP names that group and the generator asserts that
# its recorded parents indeed show none.
EXTRA = [(4, 1, 10), (4, 2, 38), (5, 2, 23)]
NO_GAP = {(5, 1)}
PS = cc.PS_A
P = max(PS)
OUT = (4, 1, 0)  # the scale-out fleet: change_cases.parent(model, 4, 1, 0)
OUT_POOL = 3
OUT_ADD = 2


def pair_key(M, k, s, pair):
    return f"{M},{k},{s},{pair[0]}-{pair[1]}"


def out_key(added):
    return "+".join(str(j) for j in added) or "none"


def pairs(M):
    return list(itertools.combinations(range(M), 2))


def out_case(model):
    """(devs, w, pool) of the scale-out case: the pool is the last three devices of a 7-device fleet."""
    devs, w = cc.parent(model, *OUT)
    return devs, w, list(bc.devices(7, 1))[4:4 + OUT_POOL]


def best(objs):
    """(index, value) of the strict earliest minimum of a list of objectives (None: no plan); (None, None) when no
    entry has a plan."""
    at, least = None, None
    for i, o in enumerate(objs):
        if o is not None and (least is None or o < least):
            at, least = i, o
    return at, least


def greedy_pair(single, pair_obj, M, p):
    """The pair a greedy repeat of the best single loss picks at budget p: the best single loss i (single[i][p]),
    then the best second device j by the pair's own value."""
    i, _ = best([single[j][p] for j in range(M)])
    if i is None:
        return None
    others = [j for j in range(M) if j != i]
    j, _ = best([pair_obj[tuple(sorted((i, j)))][p] for j in others])
    return None if j is None else tuple(sorted((i, others[j])))


def golden():
    return json.loads((GOLDEN / "scale.json").read_text())
