"""Boxes on w and n around memory-pressured and irregular optima, and their exact-oracle answers, shared by
test_pressure_box.py and test_gpu_pressure_box.py.

tests/box_cases.py builds its boxes on bounds_cases.devices, unscaled synthetic fleets on which few optima use a
slack (48 of 530 a t > 0, none of them t > n): whether n_max narrows t with n, or whether the n box is applied
before or after the capacity rows' own ends, cannot be seen there. Here the same kinds are rebuilt around the optima of
tests/pressure_cases.py and tests/irregular_cases.py ("Memory pressure and irregular fleets
under boxes, budgets and selection").

A fleet is ("p", pressure case), ("i", irregular case) or ("t", tight case), kv 4bit, on the 80-layer model; an instance is
(fleet, k, kind). The incumbent of a pressured fleet is the exact optimum of seed + 100 of the same class at the
same k; of an irregular fleet the oracle's own optimum; n clipped into the fleet's own [0, nhi_i]. Kinds: those
of box_cases ("box1", "box2", "off", "half", "pin", "cross", "nogpu"), re-based on the pressured free optimum
(w*, n*), and

  "push"   n_min_j = n*_j + 2 on the GPU device with the largest n* (the first such device), where that exceeds
           what its VRAM holds (n*_j + 2 + Kvram_j > 0; no case elsewhere): VRAM is over-subscribed there, so t_j
           must rise -- n is bound from below and t is not.
  "tcap"   the largest n_max_j strictly below the class-3 set row's lower end nL(w*_j) = w*_j + Kset_j - W, on
           the device where that end is largest and positive (no case where none is): the device's leaf is cut
           off above the w with nL(w) <= n_max_j, and is empty when nL(1) > n_max_j.

A third group, the tight fleets ("t", tight_dicts), are pressured fleets with c_cpu raised on one CUDA device until
its RAM row's lower end on n is positive, and c_gpu raised on one until Kvram = 3 > 0: the synthetic generator leaves
both at 0, so without them no fleet of the suite has nL > 0 or t > n, "tcap" has no case, and a bound on t taken
from n_max cuts off no feasible n.

The oracle is box_cases.boxed_problem's rule on pc.problem / ic.problem: lb / ub are copied, the cached dicts are
never modified. Answers are computed once per session."""

from functools import lru_cache

import numpy as np

from oracle import milp_oracle as mo

from . import box_cases as xc
from . import irregular_cases as ic
from . import pressure_cases as pc

IMAX = xc.IMAX
REL_OBJ = pc.REL_OBJ
KINDS = xc.KINDS + ("push", "tcap")
GOOD_KINDS = xc.MOVE_KINDS + xc.CAP_KINDS + ("pin", "push")  # the kinds at least half of whose instances are feasible
SEEDS = (0, 1, 2, 3)
# (M, scale) -> the k asked: M = 64 the register route's k = 1, the small fleets the table route's k
CLASSES = {(5, pc.S16): (1, 2, 4), (16, pc.S16): (1, 2, 4), (16, pc.S64): (1, 2, 4), (64, pc.S16): (1,),
           (64, pc.S64): (1,)}
# the irregular fleets taken: a device edit that touches a VRAM row, or a head edit
IRREGULAR_EDITS = ("cuda_and_metal", "metal_none", "metal_off", "m1_with_gpu", "two_heads", "head_at:last", "no_head")


def pressured_fleets(M=None, scale=None):
    return [("p", (m, sc, s, "4bit")) for (m, sc) in CLASSES for s in SEEDS
            if (M is None or m == M) and (scale is None or sc == scale)]


# edits under which ties are structural, whatever the seed (seeds 0 .. 11 of each tried: at most 14 of 18 feasible
# instances unique): m1_with_gpu gives a GPU device a zero n coefficient, cuda_no_rate likewise removes the GPU's
# rate, slow_disk_head ties the head's slack price with another device's
TIE_EDITS = ("m1_with_gpu", "cuda_no_rate", "slow_disk_head")


def tie_heavy(fleet):
    return fleet[0] == "i" and bool(set(fleet[1][4]) & set(TIE_EDITS))


def irregular_fleets(M=None):
    out = [("i", c) for c in ic.cases(Ms=(16, 64), kvs=("4bit",)) if set(c[4]) & set(IRREGULAR_EDITS)]
    return [f for f in out if M is None or f[1][0] == M]


# the tight fleets: (M, scale, seed, k at which the RAM row's offset Kset equals W)
TIGHT = ((5, pc.S16, 0, 4), (5, pc.S16, 2, 4), (16, pc.S16, 0, 4), (16, pc.S64, 1, 4), (64, pc.S16, 0, 1), (64, pc.S64, 1, 1))
VRAM_SHORT = 3  # Kvram of a tight fleet's second CUDA device


def tight_fleets(M=None):
    return [("t", (m, sc, s, "4bit", kt)) for m, sc, s, kt in TIGHT if M is None or m == M]


def tight_dicts(M, scale, seed, kt):
    """pressured_fleet(seed, M, scale) with two device edits on its first two linux_cuda devices past device 0 (both on the one, where it has one).
    The first gets c_cpu = RAM + (W_kt - 1/2) layers, so its RAM row has Kset = W_kt = L // kt: at k = kt the row
    w - n - s3 <= -Kset with s3 <= W forces n >= nL(w) = w (every layer on the GPU), a positive lower end. The
    second gets c_gpu = VRAM + 2.5 layers, so Kvram = 3: its VRAM slack is t = n + 3 > n, the one shape in which
    a bound on t taken from n_max would cut off feasible n."""
    ds = pc.pressured_fleet(seed, M, scale)
    cu = [i for i, d in enumerate(ds) if i > 0 and ic.kind(d) == "linux_cuda"]
    assert cu, (M, scale, seed)
    cu = (cu + cu)[:2]  # a fleet with one such device takes both edits on it
    bp = float(mo._bprime(pc.our_model(), pc.kv_factor("4bit")))
    a, b = ds[cu[0]], ds[cu[1]]
    a["c_cpu"] = int(a["d_avail_ram"] + (pc.L // kt - 0.5) * bp)
    b["c_gpu"] = int(b["d_avail_cuda"] + (VRAM_SHORT - 0.5) * bp)
    return ds, cu


@lru_cache(maxsize=None)
def _tight_devices(case):
    from distilp_amd.common import DeviceProfile

    return tuple(DeviceProfile.model_validate(d) for d in tight_dicts(case[0], case[1], case[2], case[4])[0])


def fleets(M=None):
    return pressured_fleets(M) + irregular_fleets(M) + tight_fleets(M)


def ks_of(fleet):
    M = fleet[1][0]
    return (1,) if M == 64 else (1, 2, 4)


def devices(fleet):
    c = fleet[1]
    if fleet[0] == "t":
        return list(_tight_devices(c))
    return pc.devices(c[2], c[0], c[1]) if fleet[0] == "p" else ic.devices(c)


def model_of(fleet):
    m = ic.model_of(fleet[1]) if fleet[0] == "i" else pc.our_model()
    assert m is pc.our_model(), fleet  # no case of the list edits the model: one model struct per GPU call
    return m


@lru_cache(maxsize=None)
def _tight_problem(case, k):
    return mo.lower_dense(devices(("t", case)), pc.our_model(), k, pc.kv_factor("4bit"))


@lru_cache(maxsize=None)
def _tight_exact(case, k):
    st, x, b1, b2, _ = mo.exact_solve(_tight_problem(case, k))
    x.setflags(write=False)
    return st, x, b1, b2


def problem(fleet, k):
    """The fleet's cached dense problem. Shared: read only."""
    if fleet[0] == "t":
        return _tight_problem(fleet[1], k)
    return (pc if fleet[0] == "p" else ic).problem(fleet[1], k)


def exact(fleet, k):
    """(status, x, best, second) of the exact oracle on the unboxed (fleet, k). Shared: read only."""
    if fleet[0] == "t":
        return _tight_exact(fleet[1], k)
    return (pc if fleet[0] == "p" else ic).exact(fleet[1], k)


def plan_of(x, M):
    return tuple(int(v) for v in np.rint(x[:M])), tuple(int(v) for v in np.rint(x[M:2 * M]))


def free_optimum(fleet, k):
    """(status, w*, n*) of the unboxed exact optimum."""
    st, x, _, _ = exact(fleet, k)
    return (st, None, None) if st != 0 else (0,) + plan_of(x, fleet[1][0])


def own_nhi(fleet, k):
    M = fleet[1][0]
    return tuple(int(v) for v in problem(fleet, k)["ub"][M:2 * M])


def incumbent(fleet, k):
    """(w1, n1): a pressured fleet's is the optimum of seed + 100 of its class, an irregular fleet's its own
    optimum; n1 clipped into the fleet's own n range."""
    if fleet[0] in "pt":
        M, sc, s, kv = fleet[1][:4]
        st, w1, n1 = free_optimum(("p", (M, sc, s + 100, kv)), k)
    else:
        st, w1, n1 = free_optimum(fleet, k)
    assert st == 0, (fleet, k)
    return w1, tuple(min(max(0, a), h) for a, h in zip(n1, own_nhi(fleet, k)))


def box(fleet, k, kind):
    """(w_min, w_max, n_min, n_max) int lists of an instance; None where the kind has no case for this fleet."""
    M = fleet[1][0]
    W = pc.L // k
    wlo, whi, nlo, nhi = [1] * M, [W] * M, [0] * M, [IMAX] * M
    if kind in xc.MOVE_KINDS or kind == "pin":
        D = {"box1": 1, "box2": 2, "pin": 0}[kind]
        w1, n1 = incumbent(fleet, k)
        wlo, whi = [max(1, w - D) for w in w1], [min(W, w + D) for w in w1]
        nlo, nhi = [max(0, n - D) for n in n1], [n + D for n in n1]
    elif kind in xc.CAP_KINDS or kind == "push":
        st, _, n = free_optimum(fleet, k)
        if st != 0:
            return None
        if kind == "off":
            nhi[int(np.argmax(n))] = 0
        elif kind == "half":
            nhi = [v // 2 for v in n]
        else:
            gpu = [i for i, h in enumerate(own_nhi(fleet, k)) if h > 0]
            if not gpu:
                return None
            j = max(gpu, key=lambda i: (n[i], -i))
            if n[j] + 2 + vram_offsets(fleet, k).get(j, -IMAX) <= 0:  # its VRAM still holds n* + 2: no push there
                return None
            nlo[j] = n[j] + 2
    elif kind == "tcap":
        st, w, _ = free_optimum(fleet, k)
        ends = {} if st != 0 else {i: w[i] + K - W for i, K in set_row_offsets(fleet, k) if w[i] + K - W > 0}
        if not ends:
            return None
        j = min(ends, key=lambda i: (-ends[i], i))  # the largest lower end, the first such device
        nhi[j] = ends[j] - 1
    elif kind == "cross":
        j = fleet[1][2] % M
        nlo[j], nhi[j] = 3, 2
    elif kind == "nogpu":
        none = [i for i, h in enumerate(own_nhi(fleet, k)) if h == 0]
        if not none:
            return None
        nlo[none[0]] = 1
    else:
        raise ValueError(kind)
    return wlo, whi, nlo, nhi


def boxed_problem(fleet, k, b):
    """box_cases.boxed_problem's rule on a copy of the cached problem's bounds."""
    p = dict(problem(fleet, k))
    M = p["M"]
    p["lb"], p["ub"] = p["lb"].copy(), p["ub"].copy()
    p["lb"][:M] = b[0]
    p["ub"][:M] = b[1]
    p["lb"][M:2 * M] = np.maximum(0, b[2])
    p["ub"][M:2 * M] = np.minimum(p["ub"][M:2 * M], b[3])
    return p


@lru_cache(maxsize=None)
def answer(fleet, k, kind):
    """None where the kind has no case, else (box, status, x, c.x, objective, margin ok) of the exact oracle on
    the boxed problem (x read only, None where infeasible)."""
    b = box(fleet, k, kind)
    if b is None:
        return None
    p = boxed_problem(fleet, k, b)
    st, x, b1, b2, _ = mo.exact_solve(p)
    if st != 0:
        return b, st, None, None, None, True
    x = np.asarray(x, float)
    x.setflags(write=False)
    return b, 0, x, float(p["c"].dot(x)), mo.objective_value(p, x), mo.uniqueness_margin_ok(b1, b2)


def instances(fleet_list=None, kinds=KINDS, ks=None):
    """[(fleet, k, kind)] that exist."""
    return [(f, k, kind) for f in (fleets() if fleet_list is None else fleet_list)
            for k in (ks_of(f) if ks is None else ks) for kind in kinds if box(f, k, kind) is not None]


def traits(fleet, k, kind):
    """(some class slack > 0, some t > 0) of a feasible instance's optimum."""
    x, M = answer(fleet, k, kind)[2], fleet[1][0]
    return bool((x[2 * M:5 * M] > 0.5).any()), bool((x[5 * M:6 * M] > 0.5).any())


def set_row_offsets(fleet, k):
    """[(device, Kset)] of the class-3 devices with a RAM row, from the dense problem alone: the row
    b'(w - n - s3) <= rhs gives s3 >= w - n + Kset, Kset = ceil(-rhs / b' - eps), and with s3 <= W the lower end
    nL(w) = w + Kset - W of n."""
    p = problem(fleet, k)
    M, A, rhs = p["M"], p["A_ub"], p["b_ub"]
    out = []
    for i in range(M):
        rows = [r for r in range(A.shape[0]) if A[r, 4 * M + i] != 0.0 and A[r, 7 * M] == 0.0]
        if rows:
            r = rows[0]
            out.append((i, int(np.ceil(-rhs[r] / A[r, i] - mo.SLACK_EPS))))
    return out


def vram_offsets(fleet, k):
    """{device: Kvram} from the dense problem alone: a VRAM row b'(n - t) <= rhs gives t >= n + Kvram,
    Kvram = ceil(-rhs / b' - eps), the largest over the device's rows."""
    p = problem(fleet, k)
    M, A, rhs = p["M"], p["A_ub"], p["b_ub"]
    out = {}
    for i in range(M):
        for r in range(A.shape[0]):
            if A[r, 5 * M + i] != 0.0 and A[r, 7 * M] == 0.0:
                out[i] = max(out.get(i, -IMAX), int(np.ceil(-rhs[r] / A[r, M + i] - mo.SLACK_EPS)))
    return out


def check_x(x, fleet, k, kind, what=""):
    """Assert a solver's x of a feasible instance is the oracle's optimum: c.x within 1e-9 relative and, where the
    optimum is unique, the w, n, s1, s2, s3 and t columns equal to the oracle's (pressure_cases.check_x's rule on
    the boxed problem)."""
    b, st, xo, cx, _, unique = answer(fleet, k, kind)
    assert st == 0, (what, fleet, k, kind)
    M = fleet[1][0]
    x = np.asarray(x[:7 * M + 1], np.float64)
    c = problem(fleet, k)["c"]
    assert pc.close(float(np.dot(c, x)), cx), (what, fleet, k, kind, float(np.dot(c, x)), cx)
    if unique:
        assert np.array_equal(x[:2 * M], np.rint(xo[:2 * M])), (what, fleet, k, kind, "w / n", x[:2 * M], xo[:2 * M])
        assert np.array_equal(x[2 * M:6 * M], np.rint(xo[2 * M:6 * M])), (
            what, fleet, k, kind, "slack / t", x[2 * M:6 * M], xo[2 * M:6 * M])
