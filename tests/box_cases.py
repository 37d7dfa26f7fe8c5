"""The boxed-sweep cases (bounds on w AND n) and their oracle answers, shared by test_box.py and test_gpu_box.py.

A case is (M, k, seed s, kind): the fleet bounds_cases.devices(M, s) on the 80-layer llama model at kv factor 0.5.
The incumbent (w1, n1) is the exact optimum of devices(M, s + 100) at the same k, n1 clipped to the device's own
[0, nhi_i] (nhi_i = W on a GPU device, else 0: the n columns' upper bounds of the lowering). Kinds:

  "box1" / "box2"  the joint move box, D = 1, 2: w in [max(1, w1 - D), min(W, w1 + D)], n in [max(0, n1 - D), n1 + D]
  "off"            n_max = 0 on the device with the largest n of the unbounded optimum (the first such device)
  "half"           n_max_i = n*_i // 2, n* the unbounded optimum's
  "pin"            both columns pinned to (w1, n1)
  "cross"          n_min = 3, n_max = 2 on device s mod M
  "nogpu"          n_min = 1 on the first device without a GPU (no such case where every device has one)

A box is four int lists (w_min, w_max, n_min, n_max) of "no bound" values (1 / W / 0 / INT32_MAX) where a kind
leaves a side alone. The oracle is the dense lowering with lb / ub of the w and n columns replaced:
lb(n) = max(0, n_min), ub(n) = min(the lowering's own, n_max)."""

import numpy as np

from oracle import milp_oracle as mo

from . import bounds_cases as bc

KV = bc.KV
IMAX = 2**31 - 1
MOVE_KINDS = ("box1", "box2")
CAP_KINDS = ("off", "half")
BAD_KINDS = ("cross", "nogpu")
KINDS = MOVE_KINDS + CAP_KINDS + ("pin",) + BAD_KINDS

_OPT = {}  # (M, k, s) -> (status, w, n) of the unbounded exact optimum of devices(M, s)
_NHI = {}  # (M, k, s) -> the n columns' own upper bounds


def free_optimum(model, M, k, s):
    if (M, k, s) not in _OPT:
        p = mo.lower_dense(list(bc.devices(M, s)), model, k, KV)
        st, x, _, _, _ = mo.exact_solve(p)
        w = n = None
        if st == 0:
            w, n = tuple(int(round(v)) for v in x[:M]), tuple(int(round(v)) for v in x[M:2 * M])
        _OPT[(M, k, s)] = (st, w, n)
        _NHI[(M, k, s)] = tuple(int(v) for v in p["ub"][M:2 * M])
    return _OPT[(M, k, s)]


def own_nhi(model, M, k, s):
    free_optimum(model, M, k, s)
    return _NHI[(M, k, s)]


def incumbent(model, M, k, s):
    """(w1, n1): the exact optimum of devices(M, s + 100) at k, n1 clipped into devices(M, s)'s own n range."""
    st, w1, n1 = free_optimum(model, M, k, s + 100)
    assert st == 0, (M, k, s)
    return w1, tuple(min(max(0, a), h) for a, h in zip(n1, own_nhi(model, M, k, s)))


def box(model, M, k, s, kind):
    """(w_min, w_max, n_min, n_max) int lists of a case; None where the kind has no case for this fleet."""
    W = int(model.L) // k
    wlo, whi, nlo, nhi = [1] * M, [W] * M, [0] * M, [IMAX] * M
    if kind in MOVE_KINDS or kind == "pin":
        D = {"box1": 1, "box2": 2, "pin": 0}[kind]
        w1, n1 = incumbent(model, M, k, s)
        wlo, whi = [max(1, w - D) for w in w1], [min(W, w + D) for w in w1]
        nlo, nhi = [max(0, n - D) for n in n1], [n + D for n in n1]
    elif kind in CAP_KINDS:
        st, _, n = free_optimum(model, M, k, s)
        if st != 0:
            return None
        if kind == "off":
            nhi[int(np.argmax(n))] = 0
        else:
            nhi = [v // 2 for v in n]
    elif kind == "cross":
        nlo[s % M], nhi[s % M] = 3, 2
    elif kind == "nogpu":
        none = [i for i, h in enumerate(own_nhi(model, M, k, s)) if h == 0]
        if not none:
            return None
        nlo[none[0]] = 1
    else:
        raise ValueError(kind)
    return wlo, whi, nlo, nhi


def boxed_problem(model, devs, k, b):
    """The dense problem of (devs, k) with the w and n columns' bounds replaced by the box b."""
    p = mo.lower_dense(list(devs), model, k, KV)
    M = p["M"]
    p["lb"][:M] = b[0]
    p["ub"][:M] = b[1]
    p["lb"][M:2 * M] = np.maximum(0, b[2])
    p["ub"][M:2 * M] = np.minimum(p["ub"][M:2 * M], b[3])
    return p


def exact_answer(model, devs, k, b):
    """(status, x, c.x, objective, margin ok) of the exact oracle on the boxed problem (x: the full solution)."""
    p = boxed_problem(model, devs, k, b)
    st, x, b1, b2, _ = mo.exact_solve(p)
    if st != 0:
        return st, None, None, None, True
    return 0, np.asarray(x, float), float(p["c"].dot(x)), mo.objective_value(p, x), mo.uniqueness_margin_ok(b1, b2)


def cases(Ms, ks, seeds, kinds):
    return [(M, k, s, kind) for M in Ms for k in ks for s in seeds for kind in kinds]


def flat(boxes, table):
    """(w_min, w_max, n_min, n_max) int32 arrays in the table's device layout from per-fleet boxes."""
    out = tuple(np.concatenate([np.asarray(b[j], np.int64) for b in boxes]).clip(-IMAX, IMAX).astype(np.int32)
                for j in range(4))
    assert len(out[0]) == table.n_devices
    return out
