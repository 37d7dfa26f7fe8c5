"""The total-move-budget cases and their two oracles, shared by test_budget.py, test_gpu_budget.py and
tests/golden/gen_budget.py.

The problem: the fixed-k MILP of (fleet, k) -- with optional [w_min, w_max] on the w columns -- plus
sum_i |w_i - w0_i| <= 2 p, i.e. sum_i max(0, w_i - w0_i) <= p (both plans sum to W). A list case is
(M, k, seed s): the fleet bounds_cases.devices(M, s) on the 80-layer llama model at kv factor 0.5, the
incumbent w0 = bounds_cases.incumbent_w (the exact optimum of the fleet of seed s + 100 at the same k).

Oracle (a), enumeration: every deviation vector d with sum d = 0 and sum d+ <= p, the exact solver with the w
columns pinned to w0 + d; the minimum is exact. Oracle (b): HiGHS at mip_gap = 0 on the dense problem with M
integer columns d_i in [0, p] and the rows w_i - d_i <= w0_i, sum d_i <= p; its w re-priced by the exact
solver with w pinned.

tests/golden/budget.json holds the answers (obj_value per point, null: infeasible); the GPU tests read it."""

import json
from itertools import product

import numpy as np

from oracle import milp_oracle as mo

from . import bounds_cases as bc
from .conftest import GOLDEN

KV = bc.KV
# list A: oracle (a) against oracle (b); list B: oracle (b) against the pinned exact solver
LIST_A = [(M, k, s) for M, ks in ((3, (1, 2)), (4, (1, 2, 4))) for k in ks for s in range(6)]
PS_A = (0, 1, 2, 3)
LIST_B = [(M, k, s) for M, ks in ((8, (1, 2)), (16, (1, 2, 4))) for k in ks for s in range(6)]
PS_B = (0, 1, 2, 4, 8)

# list P, memory-pressured fleets (tests/pressure_cases.py, kv 4bit): (M, scale, k, seed s); the incumbent is the
# pressured optimum of seed s + 100 of the same class at the same k. M = 5: oracle (a) against (b) on PS_A;
# M = 16: oracle (b) re-priced by Pinned on PS_B; one 64-device fleet at P = 2, oracle (b).
PS_P64 = (0, 1, 2)


def _list_p():
    from . import pressure_cases as pc

    out = [(5, pc.S16, k, s) for k in (1, 2, 4) for s in range(3)]
    out += [(16, pc.S16, k, s) for k in (1, 2, 4) for s in range(3)]
    out += [(16, pc.S64, k, s) for k in (1, 2) for s in range(3)]
    return out + [(64, pc.S64, 1, 0)]


LIST_P = _list_p()


def ps_of_p(M):
    return PS_A if M == 5 else PS_B if M == 16 else PS_P64


def key_p(M, scale, k, s):
    return f"{M},1/{scale.denominator},{k},{s}"


def list_p_case(M, scale, k, s):
    """(devs, w0) of a list P case."""
    from . import pressure_cases as pc

    st, x, _, _ = pc.exact((M, scale, s + 100, "4bit"), k)
    assert st == 0, (M, scale, k, s)
    return pc.devices(s, M, scale), [int(v) for v in np.rint(x[:M])]


def list_p_answer(model, M, scale, k, s):
    """(w0, {p: obj_value}, free_p) of a list P case by its oracle; for M = 5 oracle (a), asserted equal to (b)."""
    devs, w0 = list_p_case(M, scale, k, s)
    prob = problem(model, devs, k)
    pin, objs = Pinned(prob), {}
    a = enumerate_frontier(prob, w0, PS_A) if M == 5 else None
    for p in ps_of_p(M):
        b, w = highs_budget(prob, w0, p)
        assert b is not None, (M, scale, k, s, p)
        e = pin(w)
        assert e is not None and bc.rel(b, e) <= 1e-9, (M, scale, k, s, p, b, e)
        assert sum(w) == prob["W"] and sum(max(0, x - y) for x, y in zip(w, w0)) <= p
        if a is not None:
            assert a[p] is not None and bc.rel(a[p], e) <= 1e-9, (M, scale, k, s, p, a[p], e)
            e = a[p]
        objs[p] = e
    st, x, b1, b2, _ = mo.exact_solve(prob)
    assert st == 0
    free_p = sum(max(0, int(round(v)) - c) for v, c in zip(x[:M], w0))
    return w0, objs, free_p, bool(mo.uniqueness_margin_ok(b1, b2))


def key(M, k, s):
    return f"{M},{k},{s}"


def problem(model, devs, k, w_min=None, w_max=None):
    """The dense problem of (devs, k), the w columns within [max(1, w_min), min(W, w_max)]."""
    p = mo.lower_dense(list(devs), model, k, KV)
    M = p["M"]
    if w_min is not None:
        p["lb"][:M] = np.maximum(p["lb"][:M], w_min)
    if w_max is not None:
        p["ub"][:M] = np.minimum(p["ub"][:M], w_max)
    return p


class Pinned:
    """The exact solver on one problem with the w columns pinned, answers kept per w."""

    def __init__(self, prob):
        self.prob, self.M, self.seen = prob, prob["M"], {}
        self.lb, self.ub = prob["lb"][:self.M].copy(), prob["ub"][:self.M].copy()

    def __call__(self, w):
        w = tuple(int(v) for v in w)
        if w not in self.seen:
            if any(v < lo or v > hi for v, lo, hi in zip(w, self.lb, self.ub)):
                self.seen[w] = None
            else:
                q = dict(self.prob)
                q["lb"], q["ub"] = self.prob["lb"].copy(), self.prob["ub"].copy()
                q["lb"][:self.M] = w
                q["ub"][:self.M] = w
                st, x, _, _, _ = mo.exact_solve(q)
                self.seen[w] = mo.objective_value(q, x) if st == 0 else None
        return self.seen[w]


def deviations(M, p):
    """Every integer vector d of length M with sum d = 0 and sum max(0, d) <= p."""
    out = []
    for d in product(range(-p, p + 1), repeat=M):
        if sum(d) == 0 and sum(v for v in d if v > 0) <= p:
            out.append(d)
    return out


def enumerate_frontier(prob, w0, ps):
    """Oracle (a): {p: obj_value or None}."""
    pin = Pinned(prob)
    out = {}
    for p in ps:
        best = None
        for d in deviations(len(w0), p):
            o = pin([a + b for a, b in zip(w0, d)])
            if o is not None and (best is None or o < best):
                best = o
        out[p] = best
    return out


def highs_budget(prob, w0, p):
    """Oracle (b): (obj_value, w) or (None, None). The budget rows on M extra integer columns d_i."""
    M, N = prob["M"], len(prob["c"])
    q = dict(prob)
    q["c"] = np.concatenate([prob["c"], np.zeros(M)])
    q["integrality"] = np.concatenate([prob["integrality"], np.ones(M, np.uint8)])
    q["lb"] = np.concatenate([prob["lb"], np.zeros(M)])
    q["ub"] = np.concatenate([prob["ub"], np.full(M, float(p))])
    rows = np.zeros((M + 1, N + M))
    for i in range(M):
        rows[i, i] = 1.0
        rows[i, N + i] = -1.0
    rows[M, N:] = 1.0
    q["A_ub"] = np.vstack([np.hstack([prob["A_ub"], np.zeros((prob["A_ub"].shape[0], M))]), rows])
    q["b_ub"] = np.concatenate([prob["b_ub"], np.asarray(w0, float), [float(p)]])
    q["A_eq"] = np.hstack([prob["A_eq"], np.zeros((1, M))])
    res = mo.highs_solve(q, mip_gap=0.0)
    if not res.success:
        return None, None
    x = res.x[:N]
    return mo.objective_value(prob, x), [int(round(v)) for v in x[:M]]


def list_case(model, M, k, s):
    """(devs, w0) of a list case."""
    return list(bc.devices(M, s)), list(bc.incumbent_w(model, M, k, s))


# ------------------------------------------------------------------ the edge shapes (each one small launch)
def _tied_four():
    from distilp_amd.synth import load_templates, synth_fleet

    from .ties import _validate

    src = synth_fleet(21000, 16, load_templates())
    return _validate(src[:2] + src[:2])


def _spread(W, M):
    """An incumbent that is no optimum: W dealt out as evenly as it goes."""
    return [W // M + (1 if i < W % M else 0) for i in range(M)]


_EDGE = {}  # every case is on the one model


def edge_cases(model):
    """{name: dict(devs, k, w0, w_min, w_max, P, oracle)}; oracle "a" (enumeration) or "b" (HiGHS + pinned)."""
    from . import pressure_cases as pc

    if _EDGE:
        return _EDGE
    L = int(model.L)
    out = _EDGE
    out["one_device"] = dict(devs=list(bc.devices(1, 0)), k=1, w0=[L], w_min=None, w_max=None, P=2, oracle="a")
    devs, w0 = list_case(model, 64, 1, 0)
    out["wide_64"] = dict(devs=devs, k=1, w0=w0, w_min=None, w_max=None, P=2, oracle="b")
    devs, w0 = list_case(model, 4, 1, 0)
    j = int(np.argmax(w0))
    cap = [L] * 4
    cap[j] = w0[j] - 2
    out["cap_excludes_w0"] = dict(devs=devs, k=1, w0=w0, w_min=None, w_max=cap, P=3, oracle="a")
    lo, hi = [1] * 4, [L] * 4
    lo[0], hi[0] = 5, 3
    out["crossing_box"] = dict(devs=devs, k=1, w0=w0, w_min=lo, w_max=hi, P=3, oracle="a")
    devs3 = list(bc.devices(3, 1))
    W4 = L // 4
    out["clipped_window"] = dict(devs=devs3, k=4, w0=[1, 1, W4 - 2], w_min=None, w_max=None, P=3, oracle="a")
    tied = _tied_four()
    out["tied_k2"] = dict(devs=tied, k=2, w0=[L // 2 - 6, 2, 2, 2], w_min=None, w_max=None, P=3, oracle="a")
    pr = pc.devices(0, 3, pc.S16)
    out["pressured"] = dict(devs=pr, k=2, w0=_spread(L // 2, 3), w_min=None, w_max=None, P=3, oracle="a")
    # a pressured 5-device fleet around the pressured optimum of seed + 100: a cap that excludes w0, and a floor
    devs5, w5 = list_p_case(5, pc.S16, 2, 1)
    j = int(np.argmax(w5))
    cap = [L] * 5
    cap[j] = w5[j] - 2
    out["pressured_cap_excludes_w0"] = dict(devs=devs5, k=2, w0=w5, w_min=None, w_max=cap, P=3, oracle="a")
    i = int(np.argmin(w5))
    lo = [1] * 5
    lo[i] = w5[i] + 1
    out["pressured_w_min"] = dict(devs=devs5, k=2, w0=w5, w_min=lo, w_max=None, P=3, oracle="a")
    return out


def edge_answer(model, e):
    """{p: obj_value or None} for p = 0 .. P of an edge case, by its oracle."""
    prob = problem(model, e["devs"], e["k"], e["w_min"], e["w_max"])
    ps = range(e["P"] + 1)
    if e["oracle"] == "a":
        return enumerate_frontier(prob, e["w0"], ps)
    pin = Pinned(prob)
    out = {}
    for p in ps:
        o, w = highs_budget(prob, e["w0"], p)
        out[p] = None if o is None else pin(w)
    return out


def golden():
    return json.loads((GOLDEN / "budget.json").read_text())
