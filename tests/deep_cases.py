"""The budget, change and subset cases on deep models and full-wave fleets at k > 1, shared by test_deep.py,
test_gpu_deep.py and tests/golden/gen_deep.py. The oracles are budget_cases' and change_cases' own; every model is
the llama fixture with another L (model_at), the kv factor bounds_cases.KV.

Wide, k > 1 (WIDE): a parent is (kind, M, seed s, L, k): bounds_cases.devices(M, s), for kind "r" the same list
reversed, for kind "p" the memory-pressured pressure_cases.devices(s, M, 1/16). Its incumbent w is STALE, the exact
optimum of seed s + 100 of the same kind under the same model and k (bounds_cases.incumbent_w's rule; that
function's cache is per 80-layer case, so the incumbents here have their own). The budget case of a parent is the
frontier around w on the points PS_W; its change lists (wide_lists) lose the largest holder, device 0 (the head),
the last device, one device that holds a single layer, and two devices at once; the full 64-device parent also
loses its last device for a joiner from another seed. The W = M parent (L = 256, k = 4) has the all-ones plan only.

Kind "f" is constructed to pin the k > 1 threshold scan on lanes 32 .. 63: the devices sorted by their cycle time
at one layer, fastest first, around the parent's own optimum REVERSED, so the slowest devices hold the most layers.
Every optimum's cycle time T = max_i H_i then belongs to a lane >= 32 and lies above every H that lanes 0 .. 31
have anywhere in their windows (scan_witness, asserted by the generator and by test_deep.py): a scan that draws its
candidate thresholds from lanes 0 .. 31 alone never admits the optimal plan.

Deep, byte edge (deep_cases): lists of 1, 2, 3, 16 and 63 devices on the models of 320 and 512 layers whose
incumbents put 2 P + D on 254 (change.MAX_ENTRY), on 253, and some w0_i above 255; REJECTED holds the same lists
one orphaned layer further. deep_budget_cases: the budget kernel's own top (P = 63, table index 126) at L = 512.

tests/golden/deep.json holds the recorded answers (no plans); the GPU tests read it."""

import json

import numpy as np

from oracle import milp_oracle as mo

from . import bounds_cases as bc
from . import budget_cases as bu
from . import change_cases as cc
from .conftest import GOLDEN

KV = bc.KV
PS_W = (0, 1, 2, 4)
JOINER = (64, 7, 5)  # the device that joins: bounds_cases.devices(64, 7)[5]

# name: (kind, M, seed, L, k)
WIDE = {
    "w64": ("s", 64, 0, 160, 2),
    "w64r": ("r", 64, 0, 160, 2),  # w64 in reverse list order: the other half of the fleet on lanes 32 .. 63
    "f64": ("f", 64, 0, 160, 2),  # sorted fastest first, the slow half holds the most: see above
    "w48": ("s", 48, 1, 160, 2),
    "p64": ("p", 64, 0, 160, 2),
    "ones64": ("s", 64, 0, 256, 4),  # W = 64 = M: w = (1, ..., 1) is the only plan
}
FLAT = ("ones64",)  # the parents whose frontiers cannot move


def model_at(model, L):
    return model.model_copy(update={"L": int(L)})


def _devs(kind, M, s):
    if kind == "s":
        return list(bc.devices(M, s))
    if kind == "r":
        return list(reversed(bc.devices(M, s)))
    if kind == "f":
        return _fast_first(M, s)
    from . import pressure_cases as pc

    return pc.devices(s, M, pc.S16)


def cycle_tables(model, devs, k, ws):
    """[(G, H, n) per w of ws[i]] per device i: the device's objective term and cycle time at w layers with its
    cheapest n -- plans.evaluate_plan_np's per-device arithmetic, which needs a whole plan, restated for one device
    and one w at a time."""
    from distilp_amd.solver import plans as pl
    from distilp_amd.solver.fleets import fleet_table

    r = pl.plan_records(fleet_table([list(devs)], model), model, 0, KV)
    W = int(model.L) // k
    out = []
    for i in range(len(devs)):
        hs, hv = r["Kset"][i] != pl._NO_ROW, r["Kvram"][i] != pl._NO_ROW
        cls, own, pv = int(r["cls"][i]), bool(r["own"][i]), float(r["pv"][i])
        nhi = W if r["gpu"][i] else 0
        row = []
        for w in ws[i]:
            nL = max(0, w + int(r["Kset"][i]) - W) if cls == 3 and hs else 0
            nU = min(nhi, w, nhi - int(r["Kvram"][i])) if hv else min(nhi, w)
            best = None
            for n in range(nL, nU + 1):
                sc = max(0, w - (n if cls == 3 else 0) + int(r["Kset"][i])) if own else 0
                t = max(0, n + int(r["Kvram"][i]))
                g = float(r["alpha"][i]) * w + float(r["b"][i]) * n + pv * sc + pv * t
                P = float(r["alpha"][i]) * w + float(r["b"][i]) * n + pv * sc + pv * t + float(r["cst"][i])
                Q = P + float(r["p_bp"][i]) * w
                H = 0.5 * (P + Q) if Q >= P else P
                if best is None or g < best[0]:
                    best = (g, H, n)
            row.append(best)
        out.append(row)
    return out


_FAST = {}


def _fast_first(M, s):
    """bounds_cases.devices(M, s) sorted by the cycle time at one layer (L = 160, k = 2), fastest first."""
    if (M, s) not in _FAST:
        from . import pressure_cases as pc

        devs = list(bc.devices(M, s))
        tb = cycle_tables(model_at(pc.our_model(), 160), devs, 2, [[1]] * M)
        _FAST[(M, s)] = [devs[i] for i in np.argsort([row[0][1] for row in tb], kind="stable")]
    return list(_FAST[(M, s)])


def scan_witness(model, devs, k, w0, P, w):
    """(cycle time of the plan w with the exact solver's n, its bottleneck lane, the largest H that lanes 0 .. 31
    have anywhere in their windows [max(1, w0 - P), w0 + D + P]) of a list around w0."""
    from distilp_amd.solver import plans as pl
    from distilp_amd.solver.fleets import fleet_table

    M, W = len(devs), int(model.L) // k
    D = W - sum(w0)
    q = bu.problem(model, devs, k)
    q["lb"][:M] = w
    q["ub"][:M] = w
    st, x, _, _, _ = mo.exact_solve(q)
    assert st == 0
    ev = pl.evaluate_plan_np(fleet_table([list(devs)], model), model, 0, k, list(w),
                             [int(round(v)) for v in x[M:2 * M]], KV)
    tb = cycle_tables(model, devs[:32], k, [range(max(1, a - P), min(W, a + D + P) + 1) for a in w0[:32]])
    return float(ev.cycle), int(ev.bottleneck), max(e[1] for row in tb for e in row if e is not None)


def wide_devices(name):
    kind, M, s, _, _ = WIDE[name]
    return _devs(kind, M, s)


_INC = {}


def wide_incumbent(model, name):
    """The stale incumbent of a wide parent: the exact optimum of seed s + 100 under the parent's model and k (kind
    "f": see the module's text)."""
    if name not in _INC:
        kind, M, s, L, k = WIDE[name]
        # kind "f": the parent's own optimum in reverse, the most layers on the slowest devices
        src = _devs(kind, M, s) if kind == "f" else _devs(kind, M, s + 100)
        st, x, _, _, _ = mo.exact_solve(mo.lower_dense(src, model_at(model, L), k, KV))
        assert st == 0, name
        _INC[name] = [int(round(v)) for v in x[:M]][::-1 if kind == "f" else 1]
    return list(_INC[name])


def wide_lists(name, devs, w):
    """{list name: (parent devices, kept indices, w0)} of a wide parent around its incumbent w. Every list but the
    joiner's shares the one parent object `devs`."""
    M = len(devs)
    out = {}
    if name in FLAT:
        picks = {"head": 0, "last": M - 1, "two": (2, M // 2)}
    else:
        big = int(np.argmax(w))
        one = next(i for i in range(1, M - 1) if w[i] == 1 and i != big)
        picks = {"largest": big, "head": 0, "last": M - 1, "single": one, "two": (2, M // 2)}
    for n, lost in picks.items():
        keep, _, w0 = cc.lose(devs, w, lost)
        out[n] = (devs, keep, w0)
    if name == "w64":
        jm, js, ji = JOINER
        keep, _, w0 = cc.lose(devs, w, M - 1)
        out["joiner"] = (list(devs) + [bc.devices(jm, js)[ji]], keep + [M], w0 + [0])
    return out


# ------------------------------------------------------------------ deep models: the byte edge
def _case(L, k, devs, idx, w0, P, ps, oracle):
    assert len(idx) == len(w0) and max(ps) == P
    D = L // k - sum(w0)
    return dict(L=L, k=k, devs=list(devs), idx=list(idx), w0=list(w0), P=P, ps=tuple(ps), oracle=oracle, D=D,
                entry=2 * P + D)


def _full(L, k, m, s, w0, P, ps, oracle=None):
    return _case(L, k, bc.devices(m, s), range(m), w0, P, ps, oracle or ("ab" if m <= 2 else "b"))


def deep_cases():
    """{name: dict(L, k, devs (the parent), idx (the list), w0, P, ps (the recorded points), oracle, D, entry)};
    entry = 2 P + D, the largest table index the list can reach."""
    out = {}
    # L = 320, k = 1
    out["a320_1_p0_d254"] = _full(320, 1, 1, 0, [66], 0, (0,))
    out["a320_2_p1_d252"] = _full(320, 1, 2, 1, [1, 67], 1, (0, 1))
    out["a320_3_p27_d200"] = _full(320, 1, 3, 0, [10, 100, 10], 27, (0, 1, 2, 27))
    out["a320_16_p1_d252"] = _full(320, 1, 16, 0, [5] * 4 + [4] * 12, 1, (0, 1))
    out["a320_2_p0_d253"] = _full(320, 1, 2, 1, [34, 33], 0, (0,))
    out["a320_3_p27_d199"] = _full(320, 1, 3, 1, [41, 40, 40], 27, (0, 1, 2, 27))
    # 63 survivors of a 64-device fleet holding 66 layers between them: the lost device held 254
    out["a320_63_p0_d254"] = _case(320, 1, bc.devices(64, 0), range(1, 64), [2] * 3 + [1] * 60, 0, (0,), "b")
    # L = 512, k = 1: incumbents above 255 layers on one device
    out["a512_1_p0_d254"] = _full(512, 1, 1, 1, [258], 0, (0,))
    out["a512_2_p0_d254"] = _full(512, 1, 2, 0, [257, 1], 0, (0,))
    out["a512_2_p1_d252"] = _full(512, 1, 2, 1, [2, 258], 1, (0, 1))
    out["a512_3_p27_d200"] = _full(512, 1, 3, 0, [260, 30, 22], 27, (0, 1, 2, 27))
    out["a512_3_p1_d251"] = _full(512, 1, 3, 0, [2, 257, 2], 1, (0, 1))
    out["a512_2_p1_d0"] = _full(512, 1, 2, 1, [300, 212], 1, (0, 1))  # no deficit: the budget kernel's problem
    # L = 512, k = 2 (W = 256): about M R1 = 765 thresholds over (P + 1)(D + P + 1) = 1255 states at most
    out["b512_3_p4_d246"] = _full(512, 2, 3, 0, [4, 3, 3], 4, (0, 1, 2, 4))
    out["b512_2_p0_d254"] = _full(512, 2, 2, 0, [1, 1], 0, (0,))
    out["b512_3_p4_d245"] = _full(512, 2, 3, 1, [5, 3, 3], 4, (0, 1, 2, 4))
    out["b512_3_p4_d40"] = _full(512, 2, 3, 0, [10, 200, 6], 4, (0, 1, 2, 4))  # off the edge: every step improves
    return out


# one call, two items: the launch's largest deficit next to D = 0, so the first item's LQ is the slice's and the
# second's is not
PAIRS = {"pair_p1": ("a512_2_p1_d252", "a512_2_p1_d0")}


def rejected_cases():
    """{name: dict(...)}: the lists at 2 P + D = 254 with one more orphaned layer (255), and a 64-device k = 2
    list with D = 254 (its two tables alone exceed the LDS budget). `error`: what the C entry's message names."""
    out = {}
    for name, e in deep_cases().items():
        if e["entry"] != 254 or len(e["idx"]) > 16:
            continue
        w0 = list(e["w0"])
        j = int(np.argmax(w0))
        w0[j] -= 1
        r = _case(e["L"], e["k"], e["devs"], e["idx"], w0, e["P"], e["ps"], e["oracle"])
        r["error"] = "254"
        out[name + "_plus1"] = r
    r = _case(640, 2, bc.devices(64, 0), range(64), [2, 2] + [1] * 62, 0, (0,), "b")
    r["error"] = "LDS"
    out["b640_64_p0_d254"] = r
    return out


def deep_answer(model, e):
    """{p: obj_value or None} on the recorded points of a deep case, by its oracle."""
    devs = [e["devs"][j] for j in e["idx"]]
    return cc.answer(model_at(model, e["L"]), devs, e["k"], e["w0"], e["ps"], e["oracle"])


def deep_budget_cases():
    """{name: dict(L, k, devs, w0, P, ps_a (oracle (a) against (b)), top (oracle (b) re-priced))}."""
    out = {}
    for m, s, w0 in ((2, 0, [300, 212]), (3, 0, [260, 200, 52])):
        for P in (63, 62):
            out[f"m512_{m}_p{P}"] = dict(L=512, k=1, devs=list(bc.devices(m, s)), w0=list(w0), P=P, ps_a=(0, 1, 2, 3),
                                         top=P)
    return out


def deep_budget_answer(model, e):
    """{p: obj_value or None}: oracle (a) asserted equal to (b) on ps_a, oracle (b) re-priced at the top."""
    prob = bu.problem(model_at(model, e["L"]), e["devs"], e["k"])
    pin = bu.Pinned(prob)
    a = bu.enumerate_frontier(prob, e["w0"], e["ps_a"])
    out = {}
    for p in tuple(e["ps_a"]) + (e["top"],):
        b, w = bu.highs_budget(prob, e["w0"], p)
        v = None if b is None else pin(w)
        if b is not None:
            assert v is not None and bc.rel(b, v) <= 1e-9, (p, b, v)
            assert sum(w) == prob["W"] and sum(max(0, x - y) for x, y in zip(w, e["w0"])) <= p
        if p in a:
            assert (a[p] is None) == (v is None) and (v is None or bc.rel(a[p], v) <= 1e-9), (p, a[p], v)
            v = a[p]
        out[p] = v
    return out


# ------------------------------------------------------------------ subsets
# (subsets_cases fleet key, max_drop, keep): ("deep", M, seed, L, k list or None for the default one)
SUBSETS = [(("deep", 64, 0, 160, (1, 2)), 1, ()), (("deep", 16, 0, 320, None), 2, ())]


def subset_id(case):
    return f"M{case[0][1]}-L{case[0][3]}-D{case[1]}"


def golden():
    return json.loads((GOLDEN / "deep.json").read_text())
