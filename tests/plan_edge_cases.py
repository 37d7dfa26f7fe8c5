"""Shapes on both sides of every integer threshold of the fused sweep's launch plan (plan_sweep,
distilp_amd/csrc/halda.hip), and their exact-oracle answers, shared by test_plan_edges.py and
test_gpu_plan_edges.py ("Plan edges").

A shape is a Shape below: the fleet sizes, the model's L (llama_3_70b/online with L replaced, kv 4bit), the k
list, at most four distinct fleets -- pressure_cases.pressured_fleet(seed, M, scale), scale 1 and one of 1/16 or
1/32 -- the batch sizes it is run at and, per batch size, the launch plan_sweep gives it. A batch larger than the
distinct fleets repeats them (batch()), every second copy in reverse order, so that a fleet's slot in a wave or
segment is not always the same.

A case is (M, scale, seed, L, kv_bits), with a sixth entry `drop` for a leave-one-out list: one fleet on one
model; an instance is (case, k). The oracle is
oracle/halda_exact.c through mo.exact_solve(mo.lower_dense(...)), computed once per (case, k) and session
(lru_cache): read only.

The `threshold` of a shape names a plain arithmetic predicate on (sizes, L, ks, nf) (THRESHOLDS) that holds on
the "at" side and fails on the "past" side; it restates no part of plan_sweep. Importing this module loads
nothing: the two LDS-budget shapes, whose L comes from libhalda's halda_lds_bytes, are made inside the tests."""

import sys
from collections import namedtuple
from fractions import Fraction
from functools import lru_cache

from oracle import milp_oracle as mo

from . import pressure_cases as pc

KV = "4bit"
ONE, S16, S32 = Fraction(1), Fraction(1, 16), Fraction(1, 32)
LDS_BUDGET = 160 * 1024

# the launches of plan_sweep as last_fleet_ms names them: (kernels that ran, read as a set)
REG = ("halda_sweep_kernel",)                                   # kRegAlone
TABLES = ("halda_sweep_tables_kernel",)                         # kTablesAlone
REG_GATED = ("halda_sweep_kernel", "halda_sweep_tables_kernel")  # kRegGated; kRegBig by its LDS shape
KSLOT = ("halda_sweep_kslot_kernel", "halda_sweep_tables_kernel")  # kKslotGated
SEG = ("halda_sweep_seg_kernel", "halda_sweep_tables_kernel")   # kSegGated
CSR = ("halda_lower_kernel",)                                   # more than 64 k: the CSR pipeline

Shape = namedtuple("Shape", "name part sizes L ks fleets launch threshold side seg dp", defaults=(None, None))
# fleets: ((M, scale, seed), ...) at most four -- the leave-one-out shapes: (63, scale, seed, drop), the lists
# of two 64-device parents; launch: {nf: kernels} on the default path; threshold: a key of THRESHOLDS; side:
# "at" / "past"; seg, dp (part B): the kernels on the "seg" fleets path (the k-slot kernel off, so the segment
# kernel takes its batches) and on "dp" (both off)


def open_k(sizes, L, ks):
    """How many k of the list have room for the batch's smallest fleet."""
    return sum(L // k >= min(sizes) for k in ks)


def kslot_table_bytes(sizes, L, ks):
    """The G and H tables of a k-slot workgroup: per open k > 1 and for each of its four fleets, two tables of
    max M rows of R + 1 doubles, R + 1 made odd (the record, pick and split areas, a few KiB, are left out: the
    two shapes on this threshold are 24 KiB and 11 KiB away from it)."""
    return sum(4 * 2 * 8 * max(sizes) * ((L // k - min(sizes) + 1) | 1) for k in ks if k > 1 and L // k > min(sizes))


# name: (the predicate as written in DESIGN.md, the predicate on (sizes, L, ks, nf)); true on the "at" side
THRESHOLDS = {
    "lanes": ("L - min M + 1 <= 64", lambda sizes, L, ks, nf: L - min(sizes) + 1 <= 64),
    "batch": ("nf <= 64", lambda sizes, L, ks, nf: nf <= 64),
    "slots": ("open k <= 16", lambda sizes, L, ks, nf: open_k(sizes, L, ks) <= 16),
    "one_slot": ("open k <= 1", lambda sizes, L, ks, nf: open_k(sizes, L, ks) <= 1),
    "no_tables": ("open k > 1 <= 0", lambda sizes, L, ks, nf: open_k(sizes, L, [k for k in ks if k > 1]) <= 0),
    "kslot_lds": ("k-slot tables <= 160 KiB", lambda sizes, L, ks, nf: kslot_table_bytes(sizes, L, ks) <= LDS_BUDGET),
    "n_k": ("len(ks) <= 64", lambda sizes, L, ks, nf: len(ks) <= 64),
    "lds": ("table slice <= 160 KiB", lambda sizes, L, ks, nf: lds_bytes(max(sizes), L) <= LDS_BUDGET),
}


def lds_bytes(M, L):
    """The table kernel's LDS slice of a k = 1 batch of M-device fleets on L layers, as plan_sweep sizes it
    (mmax = M, R + 1 = L - M + 1, M (R + 1) + M doubles of tables): halda_lds_bytes adds one to the device
    count it derives from max_cols and M to max_tab, so it is asked with 7 (M - 1) + 1 columns and M (R + 1).
    Host arithmetic of libhalda; called from inside tests only, never while they are collected."""
    import pytest

    from distilp_amd.solver import _libhalda as lh

    if not lh.LIB_PATH.exists():
        pytest.fail(f"{lh.LIB_PATH} not built (run __graft_entry__.build())")
    r1 = L - M + 1
    return int(lh.load_library().halda_lds_bytes(7 * (M - 1) + 1, r1, M * r1, 0))


@lru_cache(maxsize=None)
def lds_edge_L(M=66):
    """The largest L at which a k = 1 batch of M-device fleets still fits the 160 KiB LDS budget."""
    L = M
    while lds_bytes(M, L + 1) <= LDS_BUDGET:
        L += 1
    return L


def _fl(M, *pairs):
    return tuple((M, sc, s) for sc, s in pairs)


FOUR = ((ONE, 0), (S16, 1), (ONE, 2), (S32, 3))
KS80 = tuple(pc.KS)
# the leave-one-out lists checked against the oracle: a 64-device parent without device `drop`
LOO_DROPS = (0, 9, 18, 27, 36, 45, 54, 63)


def _gate(name, sizes, L, fleets, nfs_launch, side):
    return Shape(name, "A", sizes, L, (1,), fleets, nfs_launch, "lanes", side)


def _b(name, sizes, L, ks, launch, threshold, side, seg, dp=TABLES):
    nfs = list(launch)
    return Shape(name, "B", sizes, L, tuple(ks), _fl(sizes[0], *FOUR), launch, threshold, side,
                 {nf: seg for nf in nfs}, {nf: dp for nf in nfs})


_MIX = ((64, ONE, 0), (48, S16, 1), (48, ONE, 2), (64, S16, 3))
_TWO64 = _fl(64, (ONE, 0), (S16, 1))
_LOO = tuple((63, sc, s, d) for _, sc, s in _TWO64 for d in LOO_DROPS)
_TWO66 = _fl(66, (ONE, 0), (S16, 1))

# every shape whose L is known without libhalda, in order; pairs: "at" then "past"
STATIC_SHAPES = (
    # ---- A: the 64-lane gate, k = 1 only
    _gate("m64_r64", (64,), 127, _fl(64, *FOUR), {2: REG, 66: REG}, "at"),
    _gate("m64_r65", (64,), 128, _fl(64, *FOUR), {2: TABLES, 66: REG_GATED}, "past"),
    _gate("mix_r64", (64, 48), 111, _MIX, {66: REG}, "at"),
    _gate("mix_r65", (64, 48), 112, _MIX, {66: REG_GATED}, "past"),
    _gate("m1_r64", (1,), 64, _fl(1, *FOUR), {2: REG, 66: REG}, "at"),
    _gate("m1_r65", (1,), 65, _fl(1, *FOUR), {2: TABLES, 66: REG_GATED}, "past"),
    _gate("m2_r64", (2,), 65, _fl(2, *FOUR), {2: REG, 66: REG}, "at"),
    _gate("m2_r65", (2,), 66, _fl(2, *FOUR), {2: TABLES, 66: REG_GATED}, "past"),
    # ---- B: the k-slot and segment kernels' edges
    _b("nf64", (16,), 80, KS80, {64: TABLES}, "batch", "at", TABLES),
    _b("nf65", (16,), 80, KS80, {65: KSLOT, 66: KSLOT, 67: KSLOT}, "batch", "past", SEG),
    # (16 k is also the most the segment kernel takes: n_k <= kSegLanes)
    _b("slots16", (4,), 80, range(1, 17), {66: KSLOT}, "slots", "at", SEG),
    _b("slots17", (4,), 80, range(1, 18), {66: TABLES}, "slots", "past", TABLES),
    _b("one_slot", (16,), 80, (2,), {66: KSLOT}, "one_slot", "at", SEG),
    _b("two_slots", (16,), 80, (2, 3), {66: KSLOT}, "one_slot", "past", SEG),
    # (79 layers: R + 1 = 64 for 16 devices, so no table launch stands behind the register launch)
    _b("no_room", (16,), 79, (1, 40), {66: REG}, "no_tables", "at", REG, REG),
    _b("closed_k", (16,), 80, (3, 7), {66: KSLOT}, "no_tables", "past", SEG),
    # the k-slot workgroup holds every open k's tables at once, the segment kernel one k's at a time: on 200
    # layers k = 2, 3 fit the k-slot launch's LDS and k = 2, 3, 4 do not, so the default path takes the segment
    # kernel
    _b("kslot_fits", (16,), 200, (2, 3), {66: KSLOT}, "kslot_lds", "at", SEG),
    _b("kslot_over", (16,), 200, (2, 3, 4), {66: SEG}, "kslot_lds", "past", SEG),
    # ---- C: the k-count gate
    Shape("k64", "C", (2,), 130, tuple(range(1, 65)), _fl(2, *FOUR), {4: TABLES}, "n_k", "at"),
    Shape("k65", "C", (2,), 130, tuple(range(1, 66)), _fl(2, *FOUR), {4: CSR}, "n_k", "past"),
    # ---- E: what hangs on the register launch alone (the first two fleets of m64_r64 / m64_r65)
    Shape("alone_r64", "E", (64,), 127, (1,), _TWO64, {2: REG}, "lanes", "at"),
    Shape("alone_r65", "E", (64,), 128, (1,), _TWO64, {2: TABLES}, "lanes", "past"),
    # the leave-one-out lists of those fleets have 63 devices: one layer fewer puts them on the same sides
    Shape("loo_r64", "E", (63,), 126, (1,), _LOO, {}, "lanes", "at"),
    Shape("loo_r65", "E", (63,), 127, (1,), _LOO, {}, "lanes", "past"),
)


@lru_cache(maxsize=None)
def lds_shapes():
    """---- D: the LDS budget (66 devices: wider than a wave, so tables from the start), at the largest L whose
    slice fits and at the next; L comes from halda_lds_bytes, so these two are made inside the tests."""
    Ld = lds_edge_L(66)
    return (Shape("lds_fits", "D", (66,), Ld, (1,), _TWO66, {2: TABLES}, "lds", "at"),
            Shape("lds_over", "D", (66,), Ld + 1, (1,), _TWO66, {2: REG_GATED}, "lds", "past"))


def shapes():
    """Every shape of the list, in order."""
    return STATIC_SHAPES + lds_shapes()


def shape(name):
    if name.startswith("lds_"):
        return next(s for s in lds_shapes() if s.name == name)
    return next(s for s in STATIC_SHAPES if s.name == name)


def predicate(sh, nf):
    """The shape's threshold evaluated on (sizes, L, ks, nf)."""
    return bool(THRESHOLDS[sh.threshold][1](sh.sizes, sh.L, sh.ks, nf))


# ------------------------------------------------------------------ cases, batches, the model
def cases_of(sh):
    """The shape's distinct fleets as cases (M, scale, seed, L, kv), in order."""
    return [f[:3] + (sh.L, KV) + f[3:] for f in sh.fleets]


def batch(sh, nf):
    """nf cases: the distinct fleets repeated, every second copy reversed."""
    d = cases_of(sh)
    out = []
    while len(out) < nf:
        out += d if (len(out) // len(d)) % 2 == 0 else d[::-1]
    return out[:nf]


def ks_with_room(sh, M):
    return [k for k in sh.ks if sh.L // k >= M]


def instances(sh_list=None):
    """[(case, k)]: every distinct (case, k) with room of the shapes, in order."""
    seen, out = set(), []
    for sh in (shapes() if sh_list is None else sh_list):
        for c in cases_of(sh):
            for k in ks_with_room(sh, c[0]):
                if (c, k) not in seen:
                    seen.add((c, k))
                    out.append((c, k))
    return out


@lru_cache(maxsize=None)
def model_of(L):
    return pc.our_model().model_copy(update={"L": L})


def devices(case):
    """The case's fleet: pressured_fleet(seed, M, scale), or, for a case with a sixth entry `drop` (the
    leave-one-out shapes), pressured_fleet(seed, M + 1, scale) without device `drop`."""
    M, sc, s = case[:3]
    if len(case) == 6:
        devs = pc.devices(s, M + 1, sc)
        return devs[:case[5]] + devs[case[5] + 1:]
    return pc.devices(s, M, sc)


kv_factor = pc.kv_factor
close = pc.close


@lru_cache(maxsize=None)
def problem(case, k):
    """The dense problem of (case, k). Shared: read only."""
    return mo.lower_dense(devices(case), model_of(case[3]), k, kv_factor(case[4]))


@lru_cache(maxsize=None)
def exact(case, k):
    """(status, x, best, second) of the exact oracle on (case, k). Shared: read only."""
    st, x, b1, b2, _ = mo.exact_solve(problem(case, k))
    x.setflags(write=False)
    return st, x, b1, b2


def unique(case, k):
    st, _, b1, b2 = exact(case, k)
    return st == 0 and mo.uniqueness_margin_ok(b1, b2)


def objective(case, k):
    return mo.objective_value(problem(case, k), exact(case, k)[1])


def best_k(case, ks):
    """(k, obj_value) of the reference's k-sweep over `ks` (ascending k, strict "<") by the exact oracle."""
    best = None
    for k in sorted(ks):
        if case[3] // k < case[0] or exact(case, k)[0] != 0:
            continue
        o = objective(case, k)
        if best is None or o < best[1]:
            best = (k, o)
    return best


def best_k_is_clear(case, ks):
    """Whether the two best objectives over the k with room differ by more than 1e-7 relative."""
    objs = sorted(objective(case, k) for k in ks if case[3] // k >= case[0] and exact(case, k)[0] == 0)
    return len(objs) < 2 or objs[1] - objs[0] > 1e-7 * max(1.0, abs(objs[0]))


def has_slack_or_t(case, k):
    st, x, _, _ = exact(case, k)
    M = case[0]
    return st == 0 and bool((x[2 * M:6 * M] > 0.5).any())


def shares(inst):
    out = {"instances": len(inst), "feasible": 0, "unique": 0, "slack_or_t": 0}
    for c, k in inst:
        if exact(c, k)[0] == 0:
            out["feasible"] += 1
            out["unique"] += unique(c, k)
            out["slack_or_t"] += has_slack_or_t(c, k)
    return out


def check_x(x, case, k, what=""):
    """pressure_cases.check_x on a case of this list: c.x within 1e-9 relative and, where the optimum is unique,
    the w, n, s1, s2, s3 and t columns equal to the oracle's."""
    pc.check_x(x, case, k, what, cases=sys.modules[__name__])
