"""The bounded-sweep cases and their oracle answers, shared by test_bounds.py and test_gpu_bounds.py.

A case is (M, k, seed s, kind): the fleet synth_fleet(s, M) on the 80-layer llama model at kv factor 0.5; the
incumbent w0 is the exact optimum of synth_fleet(s + 100, M) at the same k. kind 1 / 2: the move box
[max(1, w0 - D), min(W, w0 + D)] for D = 1, 2; kind "cap": the uniform cap w_max = ceil(W / M) + 1. The oracle
for a bounded instance is the dense lowering with the bounds of its M w columns replaced."""

from functools import lru_cache

import numpy as np

from distilp_amd.synth import synth_fleet
from oracle import milp_oracle as mo

from .helpers import synth_devices

KV = 0.5
L = 80
SEEDS = tuple(range(12))
KINDS = (1, 2, "cap")


@lru_cache(maxsize=None)
def devices(M, s):
    return synth_devices(M, s, synth_fleet(s, M))


_W0 = {}  # (M, k, s) -> the incumbent's w (every case is on the same model)


def incumbent_w(model, M, k, s):
    if (M, k, s) not in _W0:
        st, x, _, _, _ = mo.exact_solve(mo.lower_dense(list(devices(M, s + 100)), model, k, KV))
        assert st == 0, (M, k, s)
        _W0[(M, k, s)] = tuple(int(round(v)) for v in x[:M])
    return _W0[(M, k, s)]


def box(model, M, k, s, kind):
    """(lo, hi) int lists of a case."""
    W = int(model.L) // k
    if kind == "cap":
        return [1] * M, [min(W, -(-W // M) + 1)] * M
    w0 = incumbent_w(model, M, k, s)
    return [max(1, w - kind) for w in w0], [min(W, w + kind) for w in w0]


def bounded_problem(model, devs, k, lo, hi):
    """The dense problem of (devs, k) with the w columns' bounds replaced by [lo, hi]."""
    p = mo.lower_dense(list(devs), model, k, KV)
    M = p["M"]
    p["lb"][:M] = lo
    p["ub"][:M] = hi
    return p


def exact_answer(model, devs, k, lo, hi):
    """(status, w, n, c.x, objective, margin ok) of the exact oracle on the bounded problem."""
    p = bounded_problem(model, devs, k, lo, hi)
    st, x, b1, b2, _ = mo.exact_solve(p)
    if st != 0:
        return st, None, None, None, None, True
    M = p["M"]
    w = [int(round(v)) for v in x[:M]]
    n = [int(round(v)) for v in x[M:2 * M]]
    return 0, w, n, float(p["c"].dot(x)), mo.objective_value(p, x), mo.uniqueness_margin_ok(b1, b2)


def cases(Ms, ks, seeds=SEEDS, kinds=KINDS):
    return [(M, k, s, kind) for M in Ms for k in ks for s in seeds for kind in kinds]


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def flat(fleets_bounds, table):
    """(w_min, w_max) int32 arrays in the table's device layout from per-fleet (lo, hi) lists."""
    lo = np.concatenate([np.asarray(b[0], np.int32) for b in fleets_bounds])
    hi = np.concatenate([np.asarray(b[1], np.int32) for b in fleets_bounds])
    assert len(lo) == table.n_devices
    return lo, hi
