"""The change-frontier cases (a device lost or joining a live fleet) and their two oracles, shared by
test_change.py, test_gpu_change.py and tests/golden/gen_change.py.

The problem: the fixed-k MILP of a LIST of devices (a sub-fleet of a parent, in list order) -- with optional
[w_min, w_max] on the w columns -- around the layers w0_i >= 0 the listed devices hold, D = W - sum w0 >= 0 of
them orphaned: point p is the optimum over the plans with released = sum_i max(0, w0_i - w_i) <= p.

A list case is a parent (M, k, seed s) = bounds_cases.devices(M, s) on the 80-layer llama model at kv factor 0.5
whose incumbent is the parent's own exact optimum at k; each single device is lost in turn, so the items of a
parent are its M leave-one-out lists, the survivors keeping the incumbent's layers.

Oracle (a), enumeration: every deviation vector d with sum d = D, sum max(0, -d) <= p and w0_i + d_i >= 1, the
exact solver pinned on w0 + d. Oracle (b): HiGHS at mip_gap = 0 on the dense problem of the list with M integer
columns r_i >= 0, the rows w0_i - w_i - r_i <= 0 and sum r <= p; its w re-priced by the pinned exact solver.

tests/golden/change.json holds the answers (recorded results only); the GPU tests read it."""

import json

import numpy as np

from oracle import milp_oracle as mo

from . import bounds_cases as bc
from .budget_cases import Pinned, problem
from .conftest import GOLDEN

KV = bc.KV
# list A: oracle (a) against oracle (b); list B: oracle (b) re-priced by the pinned exact solver
# The seeds are picked so that every (M, k > 1) group has steps that strictly improve (gen_change.py asserts it).
# At k = 1 no seed can: the objective is separable and, where the rows are convex, the optimum of the survivors
# never takes a layer off a device that the parent's optimum gave it, so an optimal incumbent's frontier is
# flat. List S (below) therefore adds lists around a STALE incumbent, where k = 1 releases layers too.
SEEDS_A = {(4, 1): (0, 1), (4, 2): (16, 53), (4, 4): (30, 0), (5, 1): (0, 1), (5, 2): (9, 45), (5, 4): (8, 37)}
LIST_A = [(M, k, s) for (M, k), ss in SEEDS_A.items() for s in ss]
PS_A = (0, 1, 2, 3)
SEEDS_B = {(8, 1): (0,), (8, 2): (11, 3), (16, 1): (0,), (16, 2): (9,)}
LIST_B = [(M, k, s) for (M, k), ss in SEEDS_B.items() for s in ss]
PS_B = (0, 1, 2, 4, 8)
# list S: the incumbent is bounds_cases.incumbent_w, the exact optimum of the fleet of seed s + 100 (a stale
# plan), each single device lost in turn; oracle (a) against (b) on PS_A
LIST_S = [(M, k, s) for M in (4, 5) for k in (1, 2) for s in (0, 1)]
WIDE = (64, 1, 0)  # one 64-device parent, oracle (b)
PS_W = (0, 1, 2)


def _list_p():
    from . import pressure_cases as pc

    return [(5, pc.S16, 2, 0), (16, pc.S16, 2, 4)]  # two memory-pressured parents at k = 2: (M, scale, k, seed)


LIST_P = _list_p()


def ps_of(M):
    return PS_A if M <= 5 else PS_B if M <= 16 else PS_W


def key(M, k, s, lost):
    return f"{M},{k},{s},{lost}"


def key_p(M, scale, k, s, lost):
    return f"{M},1/{scale.denominator},{k},{s},{lost}"


_PARENT = {}


def parent(model, M, k, s, scale=None):
    """(devs, w) of a parent: its devices and its own exact optimum at k (the incumbent)."""
    c = (M, k, s, scale)
    if c not in _PARENT:
        if scale is None:
            devs = list(bc.devices(M, s))
        else:
            from . import pressure_cases as pc

            devs = pc.devices(s, M, scale)
        st, x, _, _, _ = mo.exact_solve(mo.lower_dense(devs, model, k, KV))
        assert st == 0, c
        _PARENT[c] = (devs, [int(round(v)) for v in x[:M]])
    return _PARENT[c]


def stale_parent(model, M, k, s):
    """(devs, w) of a list S parent: its devices and the stale incumbent."""
    return list(bc.devices(M, s)), list(bc.incumbent_w(model, M, k, s))


def lose(devs, w, lost):
    """(kept indices, listed devices, w0) of the fleet without the devices `lost` (an index or a tuple)."""
    gone = {lost} if isinstance(lost, int) else set(lost)
    keep = [i for i in range(len(devs)) if i not in gone]
    return keep, [devs[i] for i in keep], [w[i] for i in keep]


# ------------------------------------------------------------------ the oracles
def deviations(w0, D, p):
    """Every integer vector d with sum d = D, sum max(0, -d) <= p and w0_i + d_i >= 1, as (d, released)."""
    M = len(w0)
    out = []

    def rec(i, d, need, rel):
        # need: what the remaining devices must still add up to (sum of their d)
        if i == M:
            if need == 0:
                out.append((tuple(d), rel))
            return
        lo = max(-(p - rel), 1 - w0[i])
        rest = M - 1 - i
        # the remaining devices can lower the sum by at most p - rel in total, so d_i <= need + (p - rel)
        hi = need + (p - rel) if rest else need
        for v in range(lo, hi + 1):
            if rest == 0 and v != need:
                continue
            rec(i + 1, d + [v], need - v, rel + max(0, -v))

    rec(0, [], D, 0)
    return out


def enumerate_frontier(prob, w0, ps):
    """Oracle (a): {p: obj_value or None}, one pass over the vectors of the largest p."""
    pin = Pinned(prob)
    D = int(prob["W"]) - sum(w0)
    top = max(ps)
    best = [None] * (top + 1)  # by exactly r released
    for d, r in deviations(list(w0), D, top):
        o = pin([a + b for a, b in zip(w0, d)])
        if o is not None and (best[r] is None or o < best[r]):
            best[r] = o
    out = {}
    for p in ps:
        vals = [v for v in best[:p + 1] if v is not None]
        out[p] = min(vals) if vals else None
    return out


def highs_change(prob, w0, p):
    """Oracle (b): (obj_value, w) or (None, None). The release rows on M extra integer columns r_i."""
    M, N = prob["M"], len(prob["c"])
    q = dict(prob)
    q["c"] = np.concatenate([prob["c"], np.zeros(M)])
    q["integrality"] = np.concatenate([prob["integrality"], np.ones(M, np.uint8)])
    q["lb"] = np.concatenate([prob["lb"], np.zeros(M)])
    q["ub"] = np.concatenate([prob["ub"], np.full(M, float(p))])
    rows = np.zeros((M + 1, N + M))
    for i in range(M):
        rows[i, i] = -1.0  # w0_i - w_i - r_i <= 0
        rows[i, N + i] = -1.0
    rows[M, N:] = 1.0
    q["A_ub"] = np.vstack([np.hstack([prob["A_ub"], np.zeros((prob["A_ub"].shape[0], M))]), rows])
    q["b_ub"] = np.concatenate([prob["b_ub"], -np.asarray(w0, float), [float(p)]])
    q["A_eq"] = np.hstack([prob["A_eq"], np.zeros((1, M))])
    res = mo.highs_solve(q, mip_gap=0.0)
    if not res.success:
        return None, None
    x = res.x[:N]
    return mo.objective_value(prob, x), [int(round(v)) for v in x[:M]]


def released(w, w0):
    return sum(max(0, b - a) for a, b in zip(w, w0))


def answer(model, devs, k, w0, ps, oracle, w_min=None, w_max=None, tag=None):
    """{p: obj_value or None} of one list by its oracle: "a" the enumeration, "ab" the enumeration asserted equal
    to HiGHS (1e-9), "b" HiGHS re-priced by the pinned exact solver (asserted within 1e-9 of HiGHS' own value)."""
    prob = problem(model, devs, k, w_min, w_max)
    W = int(prob["W"])
    out = {}
    a = enumerate_frontier(prob, w0, ps) if "a" in oracle else None
    pin = Pinned(prob)
    for p in ps:
        if "b" in oracle:
            b, w = highs_change(prob, w0, p)
            e = None
            if b is not None:
                e = pin(w)
                assert e is not None and bc.rel(b, e) <= 1e-9, (tag, p, b, e)
                assert sum(w) == W and released(w, w0) <= p and min(w) >= 1, (tag, p, w)
            if a is not None:
                assert (a[p] is None) == (e is None), (tag, p, a[p], e)
                assert e is None or bc.rel(a[p], e) <= 1e-9, (tag, p, a[p], e)
                e = a[p]
            out[p] = e
        else:
            out[p] = a[p]
    return out


def free_optimum(model, devs, k, w0, w_min=None, w_max=None):
    """(released layers of the list's exact free optimum at k, whether that optimum is unique); (None, True)
    where the list has no plan at k."""
    prob = problem(model, devs, k, w_min, w_max)
    st, x, b1, b2, _ = mo.exact_solve(prob)
    if st != 0:
        return None, True
    return released([int(round(v)) for v in x[:prob["M"]]], w0), bool(mo.uniqueness_margin_ok(b1, b2))


# ------------------------------------------------------------------ the edge shapes (each one small launch)
_EDGE = {}


def edge_cases(model):
    """{name: dict(devs, idx, k, w0, w_min, w_max, P, oracle)}: `devs` the parent, `idx` the item's list of local
    indices, w0 / w_min / w_max in list order."""
    from . import pressure_cases as pc  # noqa: F401
    from .budget_cases import _tied_four

    if _EDGE:
        return _EDGE
    L = int(model.L)
    out = _EDGE

    def case(devs, idx, k, w0, P, w_min=None, w_max=None, oracle="ab"):
        return dict(devs=list(devs), idx=list(idx), k=k, w0=list(w0), w_min=w_min, w_max=w_max, P=P, oracle=oracle)

    devs4, w4 = parent(model, 4, 1, 0)
    j = int(np.argmax(w4))
    keep, _, w0 = lose(devs4, w4, j)
    out["largest_deficit"] = case(devs4, keep, 1, w0, 3)  # the lost device held the most layers
    devs5, w5 = parent(model, 5, 2, 0)
    h = next((i for i, d in enumerate(devs5) if d.is_head), 0)
    keep, _, w0 = lose(devs5, w5, h)
    out["lost_head"] = case(devs5, keep, 2, w0, 3)
    devs2, w2 = parent(model, 2, 1, 0)
    out["one_survivor"] = case(devs2, [0], 1, [w2[0]], 2)  # w = W is forced
    devs5b, w5b = parent(model, 5, 1, 1)
    keep, _, w0 = lose(devs5b, w5b, (1, 3))
    out["two_lost"] = case(devs5b, keep, 1, w0, 3)
    joiner = bc.devices(5, 1)[2]
    out["joiner_no_deficit"] = case(devs4 + [joiner], [0, 1, 2, 3, 4], 1, w4 + [0], 3)  # point 0 has no plan
    keep, _, w0 = lose(devs4, w4, 1)
    out["joiner_and_loss"] = case(devs4 + [joiner], keep + [4], 1, w0 + [0], 3)
    # a cap below what the largest survivor holds: it must give up two layers, so points 0 and 1 have no plan
    keep, _, w0 = lose(devs5b, w5b, 0)
    cap = [L] * len(w0)
    jj = int(np.argmax(w0))
    cap[jj] = w0[jj] - 2
    out["w_max_blocks_small_p"] = case(devs5b, keep, 1, w0, 3, w_max=cap)
    lo, hi = [1] * len(w0), [L] * len(w0)
    lo[0], hi[0] = 5, 3
    out["crossing_box"] = case(devs5b, keep, 1, w0, 3, w_min=lo, w_max=hi)
    devs3 = list(bc.devices(3, 1))
    W4 = L // 4
    out["clipped_window"] = case(devs3, [0, 1, 2], 4, [1, 1, W4 - 8], 3)  # w0 - P < 1 and w0 + D + P > W
    tied = _tied_four()
    out["tied_k2"] = case(tied, [0, 1, 2], 2, [L // 2 - 10, 2, 2], 3)
    return out


def edge_answer(model, e):
    """{p: obj_value or None} for p = 0 .. P of an edge case, by its oracle."""
    devs = [e["devs"][j] for j in e["idx"]]
    return answer(model, devs, e["k"], e["w0"], range(e["P"] + 1), e["oracle"], e["w_min"], e["w_max"])


def gate_p(ch, M, D, k):
    """The largest P the launch's gate admits for lists of M devices with a deficit of D at k (ch: the
    distilp_amd.solver.change module; -1 when no P is admitted)."""
    ok = [P for P in range(ch.MAX_P + 1)
          if 2 * P + D <= ch.MAX_ENTRY and ch.change_lds_bytes(M, P, D, k) <= ch.LDS_BUDGET]
    return max(ok) if ok else -1


def golden():
    return json.loads((GOLDEN / "change.json").read_text())
