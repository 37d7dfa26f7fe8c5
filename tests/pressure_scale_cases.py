"""Scale-in / scale-out parents under memory pressure and with irregular heads, and their oracle answers, shared by
test_pressure_scale.py, test_gpu_pressure_scale.py and tests/golden/gen_pressure_scale.py.

tests/scale_cases.py builds its parents on bounds_cases.devices, unscaled synthetic fleets: every candidate list has
a plan at every budget, no optimum uses a slack, and device 0 is the only head and is never the better device to
drop. Here the parents are

  ("p", M, scale, k, seed)   pressure_cases.devices(seed, M, scale): (5, 1/16) at k in {1, 2}, two seeds each, and
                             one (16, 1/64) at k = 2 whose `keep` leaves six devices droppable (at most 15 pairs);
  ("i", case, k)             the irregular_cases fleet of the fewest devices (kv 4bit, the unedited model) that carries
                             each of IRREGULAR_EDITS; `keep` leaves at most six devices droppable, every head and
                             every edited device among them;
  ("c", M, scale, k, seed)   a pressured parent under a w_max CAP: the droppable device that holds the most layers
                             (the first one excepted) may keep two layers fewer than it holds;
  OUT                        one (5, 1/16) fleet and a pool of three devices of another seed, max_add = 2.

Why the capped parent: the incumbent holds all W layers and no fixed-k problem of these fleets is infeasible but by
its bounds (the slacks absorb any memory shortfall), so WITHOUT bounds every candidate list of a scale-in has a plan at
p = 0 -- the survivors only gain --, and a scale-out row has a plan exactly where p reaches the number of joiners,
whatever the candidate. Under the cap the lists that keep the capped device have no plan below p = 2 and those that
drop it have one: a candidate without a plan then sits before the winner, and in another launch of a chunked run.

The incumbent is STALE: the exact optimum at k of the pressured fleet of seed + 100 of the same (M, scale), the rule
of pressure_box_cases and bounds_cases.incumbent_w. Drops are d in {0, 1, 2}; the budgets are change_cases.PS_A for
parents of at most five devices and p in {0, 1, 2} for the wider ones.

The oracle: every candidate list in subsets.candidate_lists order through change_cases.answer -- lists of at most
five survivors by oracle "ab" (the enumeration asserted equal to HiGHS), wider ones by "b" (HiGHS at gap 0 re-priced
by the pinned exact solver) --, a cell (d, p) is scale_cases.best over its candidates.

tests/golden/pressure_scale.json holds the answers (recorded results and index lists only)."""

import json

import numpy as np

from distilp_amd.solver import subsets as ss
from oracle import milp_oracle as mo

from . import change_cases as cc
from . import irregular_cases as ic
from . import pressure_cases as pc
from . import scale_cases as sx
from .budget_cases import problem
from .conftest import GOLDEN

DROPS = (0, 1, 2)
PS_WIDE = (0, 1, 2)
MAX_DROPPABLE = 6
MARGIN = 1e-9  # a cell whose best other candidate is further away than this (relative) has ONE winner
CHECKED_SHARE = 0.90

PRESSURED = [("p", 5, pc.S16, 1, 0), ("p", 5, pc.S16, 1, 1), ("p", 5, pc.S16, 2, 0), ("p", 5, pc.S16, 2, 1),
             ("p", 16, pc.S64, 2, 0)]
IRREGULAR_EDITS = ("two_heads", "no_head", "head_at:last", "cuda_and_metal")
IRREGULAR_KS = (1, 2)
# the scale-out case: (M, scale, k, seed of the fleet, seed of the pool's fleet); the pool is that fleet's last
# three devices
OUT = (5, pc.S16, 2, 2, 3)
OUT_POOL = 3
OUT_ADD = 2
CAPPED = [("c", 5, pc.S16, 2, 0)]
CAP_BELOW = 2
# Classes (a parent's key without its seed; "i": the irregular parents) without a cell of condition (a), a candidate
# without a plan before the winner: no seed of 0 .. 39 of the pressured classes has one -- nor can any, nor can an
# irregular parent: see the module's text. The generator
# asserts that the recorded parents of these classes show none; the capped parent has such cells.
NO_CASE = {"a": {"p,5,1/16,1", "p,5,1/16,2", "p,16,1/64,2", "i"}}


def irregular_case(edit):
    """The case of irregular_cases.cases with the fewest devices that carries `edit`, at kv 4bit on the unedited
    80-layer model (the first such case of that size)."""
    fit = [c for c in ic.cases(kvs=("4bit",)) if edit in c[4] and ic.model_of(c) is pc.our_model()]
    return min(fit, key=lambda c: c[0])


def irregular():
    seen, out = set(), []
    for e in IRREGULAR_EDITS:
        c = irregular_case(e)
        if c not in seen:
            seen.add(c)
            out += [("i", c, k) for k in IRREGULAR_KS if pc.L // k >= c[0]]
    return out


def parents():
    return PRESSURED + CAPPED + irregular()


def key(spec):
    if spec[0] in "pc":
        t, M, sc, k, s = spec
        return f"{t},{M},1/{sc.denominator},{k},{s}"
    _, c, k = spec
    return f"i,{c[0]},{c[1].numerator}/{c[1].denominator},{c[2]},{'+'.join(c[4])},{k}"


def class_of(name):
    """A parent key's class: the key without its seed; "i" for every irregular parent."""
    return "i" if name.startswith("i,") else name.rsplit(",", 1)[0]


def stale_w(M, scale, k, seed):
    """The incumbent's layers: the exact optimum at k of the pressured fleet of seed + 100."""
    st, x, _, _ = pc.exact((M, scale, seed + 100, "4bit"), k)
    assert st == 0, (M, scale, k, seed)
    return [int(v) for v in np.rint(x[:M])]


def heads_of(devs):
    """Every is_head device; kappa's head (device 0) where none is."""
    return [i for i, d in enumerate(devs) if d.is_head] or [0]


def parent(spec):
    """dict(devs, k, w0, droppable, keep, heads, ps, w_max) of a parent; w_max a list per device or None."""
    if spec[0] in "pc":
        _, M, sc, k, s = spec
        devs, must = pc.devices(s, M, sc), []
    else:
        _, c, k = spec
        M, sc, s = c[:3]
        devs = ic.devices(c)
        must = sorted({i for idx in ic.touched(c).values() for i in idx} | set(heads_of(devs)))
    assert len(must) <= MAX_DROPPABLE, spec
    drop = sorted(must + [i for i in range(M) if i not in must][:MAX_DROPPABLE - len(must)])
    keep = [i for i in range(M) if i not in drop]
    w0, cap = stale_w(M, sc, k, s), None
    if spec[0] == "c":
        j = max(drop[1:], key=lambda i: (w0[i], -i))
        assert w0[j] > CAP_BELOW, spec
        cap = [pc.L // k] * M
        cap[j] = w0[j] - CAP_BELOW
    return dict(devs=devs, k=k, w0=w0, droppable=drop, keep=keep, heads=heads_of(devs),
                ps=cc.PS_A if M <= 5 else PS_WIDE, w_max=cap)


def out_parent():
    """The scale-out case as a parent over devs + pool: every device of devs kept, the pool holding nothing."""
    M, sc, k, s, s2 = OUT
    devs = pc.devices(s, M, sc)
    pool = pc.devices(s2, M, sc)[M - OUT_POOL:]
    return dict(devs=devs + pool, k=k, w0=stale_w(M, sc, k, s) + [0] * OUT_POOL, droppable=list(range(M, M + OUT_POOL)),
                keep=list(range(M)), heads=heads_of(devs), ps=cc.PS_A, w_max=None, n_fleet=M, pool=pool)


def candidates(par, d):
    """[(gone, kept)] of row d, in subsets.candidate_lists order; [] where the parent cannot drop d devices."""
    M, slots = len(par["devs"]), par["droppable"]
    return [(list(g), list(kp)) for g, kp in ss.candidate_lists(M, slots, d)] if d <= min(len(slots), M - 1) else []


def oracle_of(n_listed):
    return "ab" if n_listed <= 5 else "b"


def margin(objs, at):
    """The relative distance from cell's minimum objs[at] to the best OTHER candidate; None where no other
    candidate has a plan."""
    rest = [o for i, o in enumerate(objs) if i != at and o is not None]
    return None if not rest else (min(rest) - objs[at]) / max(1.0, abs(objs[at]))


def uses_slack_or_t(model, listed, k, w0, p, want, w_max=None):
    """Whether the list's optimal plan at budget p (HiGHS' w, the pinned exact solver's x, asserted to reach the
    recorded objective) has a positive s1 / s2 / s3 or t column."""
    prob = problem(model, listed, k, None, w_max)
    b, w = cc.highs_change(prob, w0, p)
    assert b is not None
    M = prob["M"]
    q = dict(prob)
    q["lb"], q["ub"] = prob["lb"].copy(), prob["ub"].copy()
    q["lb"][:M] = w
    q["ub"][:M] = w
    st, x, _, _, _ = mo.exact_solve(q)
    assert st == 0 and abs(mo.objective_value(q, x) - want) <= 1e-9 * max(1.0, abs(want)), (w, want)
    return bool((np.asarray(x[2 * M:6 * M]) > 0.5).any())


def answer(model, par, drops=DROPS, tag=None, log=None):
    """The record of one parent: {"k", "w0", "droppable", "heads", "rows": {d: {"gone": [[...]], "obj": [{p: obj or
    None} per candidate], "cells": {p: {"obj", "at", "margin", "slack_or_t"}}}}}."""
    devs, k, w, ps, cap = par["devs"], par["k"], par["w0"], par["ps"], par["w_max"]
    of = lambda kept: None if cap is None else [cap[i] for i in kept]  # noqa: E731
    rows = {}
    for d in drops:
        cands = candidates(par, d)
        objs = []
        for gone, kept in cands:
            listed, w0 = [devs[i] for i in kept], [w[i] for i in kept]
            a = cc.answer(model, listed, k, w0, ps, oracle_of(len(kept)), w_max=of(kept), tag=(tag, gone))
            objs.append({str(p): a[p] for p in ps})
            if log:
                log(f"{tag} d={d} gone={gone}: {[a[p] for p in ps]}")
        cells = {}
        for p in ps:
            col = [o[str(p)] for o in objs]
            at, least = sx.best(col)
            cell = {"obj": least, "at": at, "margin": None, "slack_or_t": False}
            if at is not None:
                kept = cands[at][1]
                cell["margin"] = margin(col, at)
                cell["slack_or_t"] = uses_slack_or_t(model, [devs[i] for i in kept], k, [w[i] for i in kept], p, least,
                                                     of(kept))
            cells[str(p)] = cell
        rows[str(d)] = {"gone": [g for g, _ in cands], "obj": objs, "cells": cells}
    return {"k": k, "w0": list(w), "droppable": par["droppable"], "heads": par["heads"], "w_max": cap, "rows": rows}


# ------------------------------------------------------------------ the conditions, from the records alone
def conditions(gold):
    """The counts of the conditions of gen_pressure_scale.py over {key: record}:
    (a) cells with a candidate WITHOUT a plan before the winner in candidate order;
    (b) (parent, d) whose cell has no plan at a small p and one at a larger p;
    (c) cells of irregular parents whose winner drops a head;
    (d) cells whose winning plan has a positive slack or t column;
    and the feasible cells, those winner-checked (margin above MARGIN or no other candidate with a plan)."""
    out = dict(a=0, b=0, c=0, d=0, cells=0, feasible=0, checked=0, a_keys=[])
    for name, rec in gold.items():
        for d, row in rec["rows"].items():
            some = [c["obj"] is not None for c in row["cells"].values()]
            out["b"] += bool(some) and not some[0] and any(some)
            for p, c in row["cells"].items():
                out["cells"] += 1
                if c["obj"] is None:
                    continue
                out["feasible"] += 1
                out["checked"] += c["margin"] is None or c["margin"] > MARGIN
                if any(o[p] is None for o in row["obj"][:c["at"]]):
                    out["a"] += 1
                    out["a_keys"].append((name, int(d), int(p)))
                out["c"] += name.startswith("i,") and bool(set(row["gone"][c["at"]]) & set(rec["heads"]))
                out["d"] += c["slack_or_t"]
    return out


def assert_conditions(gold):
    """Every condition has a cell among the records {key: record} (the scale-in parents and "out"); no parent of a
    NO_CASE class has one of its condition; at least CHECKED_SHARE of the feasible cells are winner-checked."""
    n = conditions(gold)
    for cond in "abcd":
        assert n[cond] >= 1, (cond, n)
    assert not [c for c in n["a_keys"] if class_of(c[0]) in NO_CASE["a"]], n["a_keys"]
    assert {class_of(name) for name in gold if name != "out"} - {class_of(c[0]) for c in n["a_keys"]} == NO_CASE["a"]
    assert n["checked"] >= CHECKED_SHARE * n["feasible"], n
    return n


def records(gold):
    """{key: record} of every scale-in parent and the scale-out case ("out")."""
    return {**gold["in"], "out": gold["out"]}


def golden():
    return json.loads((GOLDEN / "pressure_scale.json").read_text())
