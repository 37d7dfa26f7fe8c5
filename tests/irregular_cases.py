"""Irregular device profiles and head placements, shared by test_irregular.py, test_gpu_irregular.py and
tests/golden/gen_irregular.py.

Every other fleet of the suite is synth_fleet, a profile folder, or a numeric edit of one: device 0 is the
only head and a mac_metal device, and a device is one of five clean kinds. Here the dicts of
pressure_cases.pressured_fleet(seed, M, scale) are edited before validation, so that the flag bits of
include/halda.h, os_class, the head's index and the row structure take the combinations the five kinds never
produce ("Irregular profiles").

A case is (M, scale, seed, kv_bits, edits); `edits` is a tuple of edit names, applied in order. A device edit
acts on the first device of index > 0 whose synthetic kind (the suffix of its name) is the one it needs and
raises LookupError when the fleet has none; every edit returns the indices it changed. Two names edit the model
instead ("f_q_no_b1", "f_out_no_b1"). An instance is (case, k). The 70-device fleets run on a 160-layer copy of
the model and the 100-device fleets on a 256-layer copy (k = 1, 2 have room: the shape of test_gpu_shapes.py whose
tables exceed the LDS budget); every other case on the 80-layer model.

The oracle is oracle/halda_exact.c through mo.exact_solve(mo.lower_dense(...)); its answers are computed once
per session (lru_cache) and must not be modified by a test."""

import sys
from fractions import Fraction
from functools import lru_cache


from oracle import milp_oracle as mo

from . import pressure_cases as pc

REL_OBJ = 1e-9
ONE, S16 = Fraction(1), Fraction(1, 16)
GiB = 1 << 30


def L_of(M):
    return 256 if M > 70 else 160 if M > 64 else 80


def ks_all(M):
    """The reference's own k list of the case's model: the proper divisors of L."""
    L = L_of(M)
    return tuple(d for d in range(1, L) if L % d == 0)


def ks_of(M):
    """The k with room (W = L // k >= M)."""
    return tuple(k for k in ks_all(M) if L_of(M) // k >= M)


# ------------------------------------------------------------------ edits
def kind(d):
    return d["name"].split("-", 1)[1]


def first(ds, *kinds):
    for i, d in enumerate(ds):
        if i > 0 and kind(d) in kinds:
            return i
    raise LookupError(f"no device of kind {kinds} past device 0")


def head_of(ds):
    """kappa's head: the first is_head device, else device 0."""
    return next((i for i, d in enumerate(ds) if d["is_head"]), 0)


def _set_heads(ds, heads):
    for i, d in enumerate(ds):
        d["is_head"] = i in heads
    return sorted(heads) or [0]


def _head_at(ds, arg):
    j = len(ds) - 1 if arg == "last" else int(arg) if arg.lstrip("-").isdigit() else first(ds, arg)
    assert 0 < j < len(ds), (arg, j)
    _set_heads(ds, {j})
    return [j]


def _metal_none(ds):
    i = first(ds, "mac_metal")
    ds[i]["d_avail_metal"] = None
    return [i]


def _metal_off(ds):
    i = first(ds, "mac_metal")
    ds[i]["has_metal"] = False
    return [i]


def _cuda_and_metal(ds):
    i = first(ds, "linux_cuda")
    d = ds[i]
    d.update(has_metal=True, sgpu_metal={q: dict(v) for q, v in ds[0]["sgpu_metal"].items()},
             T_metal=ds[0]["T_metal"], d_avail_metal=d["d_avail_cuda"] // 2)
    return [i]


def _cuda_field(field, value):
    def edit(ds):
        i = first(ds, "linux_cuda")
        ds[i][field] = value
        return [i]
    return edit


def _scpu_no_q(ds):
    q = pc.our_model().Q
    ds[1]["scpu"] = {"F32" if q != "F32" else "F16": dict(ds[1]["scpu"][q])}
    return [1]


def _sgpu_no_q(ds):
    i = first(ds, "linux_cuda")
    q = pc.our_model().Q
    ds[i]["sgpu_cuda"] = {"F32" if q != "F32" else "F16": dict(ds[i]["sgpu_cuda"][q])}
    return [i]


def _scpu_zero(ds):
    ds[1]["scpu"][pc.our_model().Q]["b_1"] = 0.0
    return [1]


def _android_swap(can, avail):
    def edit(ds):
        i = first(ds, "android")
        ds[i].update(d_bytes_can_swap=can, d_swap_avail=avail)
        return [i]
    return edit


def _slow_disk(ds):
    i = 1 if head_of(ds) != 1 else 2
    ds[i]["s_disk"] = 0.5
    return [i]


def _slow_disk_head(ds):
    i = head_of(ds)
    ds[i]["s_disk"] = 0.5
    return [i]


def _slow_gpu(ds):
    i = first(ds, "linux_cuda")
    ds[i].update(T_cuda=ds[i]["T_cpu"] / 50, t_kvcpy_gpu=0.01)
    return [i]


def _kvcpy(ds):
    i = first(ds, "linux_cuda")
    ds[i].update(t_kvcpy_cpu=0.002, t_kvcpy_gpu=0.0005)
    return [i]


def _m1_with_gpu(ds):
    i = first(ds, "linux_cuda")
    ds[i]["os_type"] = "mac_no_metal"
    return [i]


def _cgpu_over(ds):
    i = first(ds, "linux_cuda")
    ds[i]["c_gpu"] = ds[i]["d_avail_cuda"] + GiB
    return [i]


HEAD_EDITS = {
    "no_head": lambda ds: _set_heads(ds, set()),
    "two_heads": lambda ds: _set_heads(ds, {0, len(ds) - 1}),
    "all_heads": lambda ds: _set_heads(ds, set(range(len(ds)))),
}
DEVICE_EDITS = {
    "metal_none": _metal_none, "metal_off": _metal_off, "cuda_and_metal": _cuda_and_metal,
    "cuda_no_rate": _cuda_field("sgpu_cuda", None), "cuda_no_load": _cuda_field("T_cuda", None),
    "cuda_no_vram": _cuda_field("d_avail_cuda", None), "cuda_uma": _cuda_field("is_unified_mem", True),
    "scpu_no_q": _scpu_no_q, "sgpu_no_q": _sgpu_no_q, "scpu_zero": _scpu_zero,
    "android_swap": _android_swap(3 * GiB, GiB), "android_swap_rev": _android_swap(GiB, 3 * GiB),
    "slow_disk": _slow_disk, "slow_disk_head": _slow_disk_head, "slow_gpu": _slow_gpu, "kvcpy": _kvcpy,
    "m1_with_gpu": _m1_with_gpu, "cgpu_over": _cgpu_over,
}
MODEL_EDITS = ("f_q_no_b1", "f_out_no_b1")
# the head_at(j) the issue asks for: j = 1, j = M - 1, a head of each other kind, and the lanes of M = 64 / 70
HEAD_AT = ("1", "last", "linux_cuda", "android", "mac_no_metal", "31", "32", "63", "66")
EDIT_NAMES = tuple(HEAD_EDITS) + tuple(f"head_at:{a}" for a in HEAD_AT) + tuple(DEVICE_EDITS) + MODEL_EDITS


def is_head_edit(name):
    return name in HEAD_EDITS or name.startswith("head_at:")


def apply_edit(ds, name):
    """Apply one device or head edit to the dicts; the indices it acted on."""
    if name.startswith("head_at:"):
        return _head_at(ds, name.split(":", 1)[1])
    return (HEAD_EDITS.get(name) or DEVICE_EDITS[name])(ds)


def edited_fleet(seed, M, scale, edits):
    """(dicts, {edit name: indices}) of pressured_fleet(seed, M, scale) with the device and head edits applied."""
    ds = pc.pressured_fleet(seed, M, scale)
    touched = {}
    for name in edits:
        if name not in MODEL_EDITS:
            touched[name] = apply_edit(ds, name)
    return ds, touched


# ------------------------------------------------------------------ the case list
def _c(M, scale, seed, *edits, kv="4bit"):
    return (M, scale, seed, kv, tuple(edits))


CASES = (
    # M = 2: device 1 is the device every edit acts on
    _c(2, S16, 2, "head_at:1", "cuda_and_metal", "cuda_uma", "kvcpy"),
    _c(2, ONE, 5, "no_head", "metal_none", "scpu_zero"),
    _c(2, S16, 2, "all_heads", "slow_gpu", "cuda_uma", kv="fp16"),
    # M = 3
    _c(3, ONE, 2, "two_heads", "metal_off", "slow_gpu", "scpu_no_q"),
    _c(3, S16, 4, "head_at:android", "android_swap", "scpu_no_q"),
    _c(3, S16, 6, "head_at:last", "cuda_no_rate", "f_out_no_b1", kv="fp16"),
    # M = 5
    _c(5, S16, 4, "head_at:mac_no_metal", "android_swap_rev", "scpu_zero"),
    _c(5, ONE, 1, "no_head", "cuda_no_vram", "metal_none", "f_q_no_b1"),
    _c(5, S16, 6, "head_at:linux_cuda", "cuda_and_metal", "kvcpy", "metal_off", "android_swap", kv="fp16"),
    _c(5, ONE, 3, "all_heads", "cgpu_over", "sgpu_no_q"),
    # M = 16: one or two edits a case, so that a failure names its edit
    _c(16, S16, 1, "no_head", "metal_none"),
    _c(16, ONE, 1, "head_at:1", "metal_off"),
    _c(16, S16, 2, "head_at:last", "cuda_no_rate"),
    _c(16, S16, 1, "head_at:linux_cuda", "cuda_and_metal", "cuda_uma"),
    _c(16, ONE, 3, "head_at:android", "android_swap"),
    _c(16, S16, 4, "head_at:mac_no_metal", "m1_with_gpu"),
    _c(16, S16, 6, "two_heads", "cuda_no_load", kv="fp16"),
    _c(16, ONE, 2, "all_heads", "cuda_no_vram"),
    _c(16, S16, 1, "scpu_no_q"),
    _c(16, ONE, 6, "sgpu_no_q", kv="fp16"),
    _c(16, S16, 2, "scpu_zero"),
    _c(16, S16, 3, "android_swap_rev", kv="fp16"),
    _c(16, ONE, 4, "slow_disk"),
    _c(16, S16, 6, "head_at:last", "slow_disk_head"),
    _c(16, S16, 1, "slow_gpu", kv="fp16"),
    _c(16, ONE, 2, "kvcpy"),
    _c(16, S16, 4, "cgpu_over", kv="fp16"),
    _c(16, S16, 6, "f_q_no_b1"),
    _c(16, ONE, 1, "head_at:1", "f_out_no_b1", kv="fp16"),
    _c(16, S16, 2, "cuda_and_metal"),
    _c(16, ONE, 6, "m1_with_gpu"),
    _c(16, S16, 3, "head_at:last", "metal_off", "cuda_uma", "android_swap", "scpu_zero"),
    # M = 33: the table kernel's second half-wave
    _c(33, S16, 1, "head_at:32", "cuda_and_metal", "metal_none", "slow_disk"),
    _c(33, ONE, 2, "no_head", "m1_with_gpu", "android_swap"),
    _c(33, S16, 3, "two_heads", "slow_gpu", "scpu_no_q", kv="fp16"),
    _c(33, ONE, 6, "head_at:31", "cuda_no_rate", "metal_off", kv="fp16"),
    _c(33, S16, 4, "all_heads", "cuda_uma", "cgpu_over", "android_swap_rev"),
    # M = 64, k = 1: the register sweep; the head on lanes 1, 31, 32 and 63
    _c(64, S16, 0, "head_at:1", "cuda_and_metal"),
    _c(64, S16, 1, "head_at:31", "metal_none", "slow_gpu"),
    _c(64, ONE, 2, "head_at:32", "m1_with_gpu"),
    _c(64, S16, 3, "head_at:63", "cuda_no_rate", "android_swap", "slow_disk_head"),
    _c(64, S16, 4, "no_head", "metal_off", "scpu_zero", kv="fp16"),
    _c(64, ONE, 6, "two_heads", "cuda_uma", "kvcpy"),
    _c(64, S16, 1, "all_heads", "cuda_no_vram", "sgpu_no_q"),
    _c(64, S16, 2, "head_at:linux_cuda", "cuda_and_metal", "cuda_uma", "f_out_no_b1", kv="fp16"),
    # M = 70 on 160 layers: global tables, the second chunk of fleet_offsets
    _c(70, S16, 1, "head_at:66", "cuda_and_metal", "metal_none", "android_swap"),
    _c(70, S16, 2, "no_head", "m1_with_gpu", "slow_gpu"),
    # M = 100 on 256 layers: tables beyond the LDS budget (the global-table kernels)
    _c(100, S16, 3, "head_at:last", "cuda_and_metal", "cuda_uma", "android_swap"),
    _c(100, S16, 4, "no_head", "m1_with_gpu", "metal_off", "slow_gpu"),
)


def cases(Ms=None, kvs=("4bit", "fp16")):
    return [c for c in CASES if (Ms is None or c[0] in Ms) and c[3] in kvs]


def instances(case_list=None):
    return [(c, k) for c in (CASES if case_list is None else case_list) for k in ks_of(c[0])]


# ------------------------------------------------------------------ shared, read-only
def edited_model(model, case):
    """`model` as the case asks: L = 160 for the fleets wider than 64 devices, f_q / f_out without "b_1" under
    the two model edits."""
    upd = {}
    if L_of(case[0]) != model.L:
        upd["L"] = L_of(case[0])
    for name, field in (("f_q_no_b1", "f_q"), ("f_out_no_b1", "f_out")):
        if name in case[4]:
            upd[field] = {b: v for b, v in getattr(model, field).items() if b != "b_1"}
    return model.model_copy(update=upd) if upd else model


@lru_cache(maxsize=None)
def model_of(case):
    """The model of a case: llama_3_70b/online, edited_model."""
    return edited_model(pc.our_model(), case)


@lru_cache(maxsize=None)
def _devices(case):
    from distilp_amd.common import DeviceProfile

    M, scale, seed, _, edits = case
    return tuple(DeviceProfile.model_validate(d) for d in edited_fleet(seed, M, scale, edits)[0])


def devices(case):
    return list(_devices(case))


def touched(case):
    M, scale, seed, _, edits = case
    return edited_fleet(seed, M, scale, edits)[1]


kv_factor = pc.kv_factor


@lru_cache(maxsize=None)
def problem(case, k):
    """The dense problem of (case, k). Shared: read only."""
    return mo.lower_dense(devices(case), model_of(case), k, kv_factor(case[3]))


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


def best_k(case, ks=None):
    """(k, obj_value) of the reference's k-sweep (ascending k, strict "<") by the exact oracle, or None."""
    best = None
    for k in sorted(ks_of(case[0]) if ks is None else ks):
        if L_of(case[0]) // k < case[0] or exact(case, k)[0] != 0:
            continue
        o = objective(case, k)
        if best is None or o < best[1]:
            best = (k, o)
    return best


def best_k_is_clear(case):
    """Whether the two best objectives over the k with room differ by more than 1e-7 relative."""
    objs = sorted(objective(case, k) for k in ks_of(case[0]) if exact(case, k)[0] == 0)
    return len(objs) < 2 or objs[1] - objs[0] > 1e-7 * max(1.0, abs(objs[0]))


def has_slack_or_t(case, k):
    st, x, _, _ = exact(case, k)
    M = case[0]
    return st == 0 and bool((x[2 * M:6 * M] > 0.5).any())


def shares(inst=None):
    inst = instances() if inst is None else inst
    out = {"instances": len(inst), "supported": 0, "feasible": 0, "unique": 0, "slack_or_t": 0}
    for c, k in inst:
        st = exact(c, k)[0]
        out["supported"] += st >= 0
        if st == 0:
            out["feasible"] += 1
            out["unique"] += unique(c, k)
            out["slack_or_t"] += has_slack_or_t(c, k)
    return out


close = pc.close


def check_x(x, case, k, what=""):
    """pressure_cases.check_x on a case of this list: c.x within 1e-9 relative and, where the optimum is unique,
    the w, n, s1, s2, s3 and t columns equal to the oracle's."""
    pc.check_x(x, case, k, what, cases=sys.modules[__name__])


@lru_cache(maxsize=None)
def exact_sweep(case):
    """(best, per_k) of the exact oracle's k-sweep of a case over the reference's own k list."""
    return mo.halda_solve_oracle(devices(case), model_of(case), mip_gap=1e-4, kv_bits=case[3], solver="exact")


def price_fixed(case, k, w, n):
    """(success, obj_value or None) of HiGHS on (case, k) with the w and n columns fixed to the plan."""
    return pc.price_fixed(case, k, w, n, prob=problem(case, k))


def neighbours(rng, w, n):
    """Two single-layer neighbours of (w, n), drawn as tests/golden/gen_plans.py draws its six: its first
    "move" (one layer from one device to another) and its first "n_plus" (n_i + 1)."""
    six = pc.neighbours(rng, w, n)
    return [six[0], six[2]]


# ------------------------------------------------------------------ tests/golden/irregular.json
def golden_cases():
    """The cases recorded in irregular.json: every case of at most 16 devices, as kv 4bit (every edit name but
    the head lanes of the wide fleets occurs among them)."""
    seen, out = set(), []
    for c in CASES:
        g = c[:3] + ("4bit",) + c[4:]
        if c[0] <= 16 and g not in seen:
            seen.add(g)
            out.append(g)
    return out


def case_of_record(rec):
    return (rec["M"], Fraction(*rec["scale"]), rec["seed"], "4bit", tuple(rec["edits"]))


def golden_mismatch(rec, solver):
    """oracle.milp_oracle's k-sweep by `solver` ("exact" / "highs") on a recorded fleet against the record
    (pressure_cases.sweep_mismatch): None when they agree, else what differs."""
    case = case_of_record(rec)
    return pc.sweep_mismatch(devices(case), model_of(case), rec, solver)
